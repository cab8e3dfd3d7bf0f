"""
Engine — thin object wrapper over the C ABI (include/rsf_abi.h).

One Engine owns one rsf_ctx.  With mem="host" every array argument is a NumPy array and calls
are synchronous; with mem="device" arguments are torch CUDA tensors (PyTorch is used only for
device memory and streams) and the work is ordered on the current torch stream.

The class is library-agnostic (`lib` is any handle typed by _abi.bind) so the test-suite can
drive the CPU oracle through the very same code; the product always passes _abi.load().
"""
import contextlib
import ctypes
import math
import os

import numpy as np

if __package__:
    from . import _abi
else:  # flat layout: this directory on sys.path, the reference's own import style (main.py:44-46)
    import _abi


def _host(x):
    """A contiguous float64 NumPy array of x (a torch tensor is copied to the host)."""
    return np.ascontiguousarray(np.asarray(x.cpu() if hasattr(x, "cpu") else x, dtype=np.float64))


def _dp(a):
    """The double* of a float64 NumPy array."""
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _i32p(a):
    """The int32_t* of an int32 NumPy array."""
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def _vec(x, d, what):
    """x, a scalar or d values, as a contiguous float64 (d,)."""
    x = np.asarray(x, dtype=np.float64)
    if x.shape not in ((), (1,), (d,)):
        raise ValueError(f"{what} has shape {x.shape}: a scalar or {d} values")
    return np.ascontiguousarray(np.broadcast_to(x, (d,)))


def _probs(p, open_interval, allow_empty, what):
    """Probabilities as a contiguous 1-D float64 array, in [0, 1] or with open_interval in (0, 1); None leaves the range to the library."""
    p = np.ascontiguousarray(np.atleast_1d(np.asarray(p, dtype=np.float64)))
    if p.ndim != 1 or not (p.size or allow_empty):
        raise ValueError(f"{what} is a {'' if allow_empty else 'non-empty '}sequence of probabilities")
    if open_interval is not None and not np.all((p > 0.0) & (p < 1.0) if open_interval else (p >= 0.0) & (p <= 1.0)):
        raise ValueError(f"{what}: probabilities lie {'strictly inside (0, 1)' if open_interval else 'in [0, 1]'}")
    return p


def _batched_probs(probs, rows, call):
    """call(pj, oj) fills the block oj (len(pj), rows) of the result (len(probs), rows), at most PREDICT_MAX_PROBS probabilities at a time."""
    out = np.empty((probs.size, rows))
    for j in range(0, probs.size, _abi.PREDICT_MAX_PROBS):
        call(probs[j:j + _abi.PREDICT_MAX_PROBS], out[j:j + _abi.PREDICT_MAX_PROBS])
    return out


def _rows_totals(out, tot, row_names, total_names):
    """Per-row columns of out as arrays and the totals as floats, by name."""
    res = {name: np.ascontiguousarray(out[:, j]) for j, name in enumerate(row_names)}
    res.update({name: float(v) for name, v in zip(total_names, tot)})
    return res


def _series_args(x, std2=None, data=None):
    """(rows, n) of a materialised series (nout, n), whose draws' std2 is (n,) and whose observation is (rows,)."""
    if x.ndim != 2 or int(x.shape[0]) < 1 or int(x.shape[1]) < 1:
        raise ValueError("a series is (nout, n)")
    rows, n = int(x.shape[0]), int(x.shape[1])
    if std2 is not None and (std2.ndim != 1 or int(std2.shape[0]) != n):
        raise ValueError(f"std2 has shape {tuple(std2.shape)}, the series has {n} draws")
    if data is not None and (data.ndim != 1 or int(data.shape[0]) != rows):
        raise ValueError(f"data has shape {tuple(data.shape)}, the series has {rows} rows")
    return rows, n


def _lag_blocks(N, lag_block, partials, finish, complete):
    """Partials of the lags [0, end), end growing by lag_block, until complete(finish(partials)) (Geyer's truncation reached
    everywhere) or every lag [0, N) is in → (partials, what finish made of them)."""
    part = None
    while True:
        end = 0 if part is None else part.shape[-1] - _abi.DIAG_HEAD
        new = partials(end, min(N, end + int(lag_block)))
        part = new if part is None else np.concatenate([part, new[..., _abi.DIAG_HEAD:]], axis=-1)
        res = finish(part)
        if part.shape[-1] - _abi.DIAG_HEAD >= N or complete(res):
            return part, res


def _model_struct(model, substeps):
    m = _abi.Model()
    m.size = ctypes.sizeof(_abi.Model)
    m.flags = _abi.FLAG_RADIATION_DAMPING if getattr(model, "RadiationDamping", True) else 0
    precision = getattr(model, "precision", "float64")
    if precision not in ("float64", "float32"):
        raise ValueError(f"precision must be 'float64' or 'float32', not {precision!r}")
    if precision == "float32":
        m.flags |= _abi.FLAG_FP32_SOLVE
    integrator = getattr(model, "integrator", "rk4")
    if integrator not in ("rk4", "dop853"):
        raise ValueError(f"integrator must be 'rk4' or 'dop853', not {integrator!r}")
    if integrator == "dop853":
        if precision != "float64":
            raise ValueError("the dop853 integrator is float64 only")
        m.flags |= _abi.FLAG_DOP853
    m.nsteps = int(model.num_tsteps)
    # the reference steps by its `delta_t` attribute and counts floor((t_final - t_start)/delta_t) samples
    # (RateStateModel.py:176,358); the C ABI derives delta_t from (t_start, t_final, num_tsteps), so a model whose
    # delta_t was edited out of step with them would silently integrate something else here: refuse it
    dt_attr = getattr(model, "delta_t", None)
    if dt_attr is not None:
        dt = (float(model.t_final) - float(model.t_start)) / m.nsteps
        if abs(float(dt_attr) - dt) > 1e-12 * abs(dt):
            raise ValueError(f"model.delta_t = {dt_attr!r} is not (t_final - t_start)/num_tsteps = {dt!r}; "
                             "set t_start, t_final, num_tsteps and delta_t consistently")
    m.substeps = int(substeps)
    m.t_start, m.t_final = float(model.t_start), float(model.t_final)
    m.mu_ref, m.V_ref, m.k1 = float(model.mu_ref), float(model.V_ref), float(model.k1)
    m.mu_t_zero = float(model.mu_t_zero)
    m.a, m.b = float(model.a), float(model.b)
    return m


def law_name(law):
    """'aging' or 'slip' of a state law's name ('ageing' is accepted)"""
    if not isinstance(law, str) or law not in _abi.LAWS:
        raise ValueError(f"state_law is 'aging' (or 'ageing') or 'slip', not {law!r}")
    return "slip" if _abi.LAWS[law] == _abi.LAW_SLIP else "aging"


def state_law_of(model):
    """The model's state evolution law, "aging" (the default) or "slip"."""
    return law_name(getattr(model, "state_law", "aging"))


_OBSERVABLE_NAMES = {_abi.OBS_ACC: "acc", _abi.OBS_MU: "mu", _abi.OBS_THETA: "theta", _abi.OBS_VELOCITY: "velocity"}


def observable_name(observable):
    """'acc', 'mu', 'theta' or 'velocity' of an observable's name ('friction', 'state' and 'V' are accepted)"""
    if not isinstance(observable, str) or observable not in _abi.OBSERVABLES:
        raise ValueError(f"observable is 'acc', 'mu' (or 'friction'), 'theta' (or 'state') or 'velocity' (or 'V'), not {observable!r}")
    return _OBSERVABLE_NAMES[_abi.OBSERVABLES[observable]]


def observable_of(model):
    """The series the model returns and is fitted to: "acc" (the default, the reference's), "mu", "theta" or "velocity"."""
    return observable_name(getattr(model, "observable", "acc"))


def stiffness_of(model):
    """The stiffness of the apparatus, independent of Dc: None (the reference's coupling k' = 0.1 / Dc) or a finite float > 0."""
    k = getattr(model, "stiffness", None)
    if k is None:
        return None
    if isinstance(k, (bool, str)) or not np.isscalar(k) or not (math.isfinite(float(k)) and float(k) > 0.0):
        raise ValueError(f"stiffness is None (the reference's coupling k' = 0.1 / Dc) or a finite float > 0, not {k!r}")
    return float(k)


_COUPLED = "the kernel integrates k' = 0.1 / Dc"


def check_law_options(model):
    """The slip law, a caller's loading history, an observable other than the acceleration and a stiffness independent of Dc run
    the float64 RK4 only → the model's law."""
    law, obs, k = state_law_of(model), observable_of(model), stiffness_of(model)
    integrator, precision = getattr(model, "integrator", "rk4"), getattr(model, "precision", "float64")
    for what, on in ((f"state_law={law!r}", law == "slip"), ("a custom loading history", getattr(model, "loading", None) is not None),
                     (f"stiffness={k!r}", k is not None)):
        if on and integrator == "dop853":
            raise NotImplementedError(f"{what} with integrator='dop853': the adaptive steps evaluate the built-in history and the ageing law")
        if on and precision == "float32":
            raise NotImplementedError(f"{what} with precision='float32': the float32 solve runs the built-in history and the ageing law")
    if obs != "acc" and integrator == "dop853":
        raise NotImplementedError(f"observable={obs!r} with integrator='dop853': the observables are samples of the float64 RK4 solve (law_observe)")
    if obs != "acc" and precision == "float32":
        raise NotImplementedError(f"observable={obs!r} with precision='float32': the observables are samples of the float64 RK4 solve (law_observe)")
    return law


def _pop_array(x, P, dtype, what):
    """x, a scalar or P values, as a contiguous (P,) array of dtype: one entry per SMC population."""
    x = np.asarray(x)
    if x.shape not in ((), (1,), (P,)):
        raise ValueError(f"{what} has shape {x.shape}: a scalar or one entry for each of the {P} populations")
    return np.ascontiguousarray(np.broadcast_to(x, (P,)).astype(dtype))


def _ptr_of(a, ctype):
    return a.ctypes.data_as(ctypes.POINTER(ctype))


def smc_batch_populations(n_groups, groups=None, seeds=None, offsets=None, replicates=1):
    """The populations of Engine.smc_batch: every group of `groups` (rows of the (n_groups, nout) data; default all) x `replicates`,
    the replicates of a group next to each other → dict(group (P,) int32 — the data row —, replicate (P,) int64, seed (P,) uint64,
    offset (P,) int64).  seeds: None or an integer seed0 (default 0) — replicate r then has seed0 + r, what a loop over
    Engine.smc(seed=...) uses — or one seed per replicate; offsets: a scalar (default 0) or one per replicate.  Pure NumPy."""
    n_groups, R = int(n_groups), int(replicates)
    if n_groups < 1 or R < 1:
        raise ValueError("need at least one data row and replicates >= 1")
    g = np.arange(n_groups) if groups is None else np.atleast_1d(np.asarray(groups))
    if g.ndim != 1 or g.size < 1 or not np.issubdtype(g.dtype, np.integer) or g.min() < 0 or g.max() >= n_groups:
        raise ValueError(f"groups is a non-empty sequence of data rows in 0..{n_groups - 1}")
    if g.size * R > _abi.SMC_BATCH_MAX:
        raise ValueError(f"{g.size} groups x {R} replicates exceed the {_abi.SMC_BATCH_MAX} populations of one call")
    sd, off = np.asarray(0 if seeds is None else seeds), np.asarray(0 if offsets is None else offsets)
    sd = int(sd) + np.arange(R) if sd.ndim == 0 else sd
    off = np.full(R, int(off)) if off.ndim == 0 else off
    if sd.shape != (R,) or off.shape != (R,):
        raise ValueError(f"seeds and offsets are a scalar or one entry per replicate ({R})")
    if (sd < 0).any() or (off < 0).any():
        raise ValueError("seeds and offsets are >= 0")
    return {"group": np.repeat(g, R).astype(np.int32), "replicate": np.tile(np.arange(R), g.size).astype(np.int64),
            "seed": np.tile(sd, g.size).astype(np.uint64), "offset": np.tile(off, g.size).astype(np.int64)}


def smc_batch_summary(log_evidence, group):
    """log p(y | M) of replicate SMC runs, per group: log_evidence (P,) and the group (P,) each belongs to → a list, in order of
    first appearance, of dict(group, replicates, log_evidence_mean — the logarithm of the mean evidence (log-mean-exp: the evidence
    estimate is unbiased, its logarithm is not) —, log_evidence_sd — the sample standard deviation (ddof = 1) of the replicates'
    log evidences —, log_evidence_se — the standard error of log_evidence_mean by the delta method, sd(Z_r / mean Z) / sqrt(R)).
    One replicate: sd and se are NaN.  Pure NumPy."""
    le, g = np.asarray(log_evidence, dtype=np.float64).reshape(-1), np.asarray(group).reshape(-1)
    if le.size != g.size or le.size < 1:
        raise ValueError("one group label for each log evidence, at least one")
    out = []
    for key in dict.fromkeys(g.tolist()):
        x = le[g == key]
        R, top = x.size, x.max()
        ratio = np.exp(x - top)  # in (0, 1], the largest exactly 1
        mean = top + np.log(ratio.mean())
        rel = ratio / ratio.mean()
        out.append({"group": key, "replicates": int(R), "log_evidence_mean": float(mean),
                    "log_evidence_sd": float(x.std(ddof=1)) if R > 1 else float("nan"),
                    "log_evidence_se": float(rel.std(ddof=1) / np.sqrt(R)) if R > 1 else float("nan")})
    return out


class _DeltaSearch:
    """The search of Engine.smc_next_delta for one population, SMC_ROUNDS rounds of 16-section: candidates() → the steps of the next
    read of l, update(res) with that read's smc_weight_sums → True once `out`, smc_next_delta's result, is there."""

    def __init__(self, lib, beta, ess_fraction):
        self.lib, self.beta, self.rho = lib, float(beta), float(ess_fraction)
        self.a, self.b, self.last, self.fail, self.rnd, self.cand, self.out = 0.0, 1.0 - float(beta), None, None, 0, None, None

    def candidates(self):
        m = _abi.SMC_MAX_CANDIDATES
        self.cand = [self.a + (self.b - self.a) * j / m for j in range(1, m + 1)]
        return self.cand

    def update(self, res):
        m, cand, sums = _abi.SMC_MAX_CANDIDATES, self.cand, res["sums"]
        k = ctypes.c_int32()
        _abi.check(self.lib, self.lib.rsf_smc_section(self.rho * res["n_finite"], m, _dp(np.ascontiguousarray(sums)), ctypes.byref(k)))
        k = k.value
        if k:
            self.last = (cand[k - 1], sums[k - 1])
        if k == m and self.rnd == 0:
            self.out = {"delta": self.b, "beta": 1.0, "lmax": res["lmax"], "sum_w": float(sums[-1, 0]), "ess": float(sums[-1, 0] ** 2 / sums[-1, 1])}
            return True
        if k < m:
            self.fail = (cand[k], sums[k])
            self.a, self.b = (cand[k - 1] if k else self.a), cand[k]
        self.rnd += 1
        if k == m or self.rnd == _abi.SMC_ROUNDS:
            delta, sw = self.last if self.last is not None else self.fail
            self.out = {"delta": delta, "beta": self.beta + delta, "lmax": res["lmax"], "sum_w": float(sw[0]), "ess": float(sw[0] ** 2 / sw[1])}
            return True
        return False


def bayes_factor(ev_a, ev_b):
    """The log Bayes factor of two results of Engine.evidence / evidence_from_ssq / PosteriorPool.evidence, model a against model
    b, for the SAME observation → dict(log_bf = log_evidence_a - log_evidence_b, re = sqrt(re_a^2 + re_b^2), the approximate
    relative error of the ratio of the two marginal likelihoods, i.e. the absolute error of log_bf).  Two results whose `shape`
    or data length `n_data` differ do not belong to one data set and are refused."""
    for key in ("shape", "n_data"):
        if ev_a[key] != ev_b[key]:
            raise ValueError(f"the two results differ in {key} ({ev_a[key]!r} against {ev_b[key]!r}): not the same observation")
    if ev_a["log_evidence"] is None or ev_b["log_evidence"] is None:
        raise ValueError("a result without log_evidence (no box given)")
    return {"log_bf": float(ev_a["log_evidence"] - ev_b["log_evidence"]), "re": float(np.hypot(ev_a["re"], ev_b["re"]))}


class FitResult:
    """Result of Engine.fit / Engine.fit_from_residuals: per start the point q (n, d), its sum of squares ssq (n,), grad = X^T r
    (n, d), jtj = X^T X (n, d, d), the damping lam (n,), status (n,) int32 (_abi.FIT_RUNNING / _CONVERGED / _STALLED / _FAILED) and
    iters (n,) int32, NumPy arrays on the host; n_groups observation series (the starts split evenly over them in order) of n_obs
    samples each.  At d = 3 the problem has a ridge (Dc a = const): a start's q is ONE POINT ON IT — compare ssq and Dc a, not the
    three parameters."""

    def __init__(self, lib, q, ssq, grad, jtj, lam, status, iters, n_groups, n_obs):
        self._lib = lib
        self.q, self.ssq, self.grad, self.jtj, self.lam, self.status, self.iters = q, ssq, grad, jtj, lam, status, iters
        self.n_groups, self.n_obs = int(n_groups), int(n_obs)

    def best(self, group=None):
        """The index of the start with the smallest finite ssq among those that are not FAILED — of observation group `group`, or
        of all starts."""
        n = self.ssq.shape[0]
        per = n // self.n_groups
        if group is not None and not 0 <= int(group) < self.n_groups:
            raise ValueError(f"group {group} is outside 0..{self.n_groups - 1}")
        idx = np.arange(n) if group is None else np.arange(int(group) * per, (int(group) + 1) * per)
        idx = idx[(self.status[idx] != _abi.FIT_FAILED) & np.isfinite(self.ssq[idx])]
        if idx.size == 0:
            raise _abi.RsfError(-1, "FitResult.best: no start has a finite sum of squares")
        return int(idx[np.argmin(self.ssq[idx])])

    def _laplace(self, shape, lo, hi, i):
        i = self.best() if i is None else int(i)
        d = int(self.q.shape[1])
        out = np.empty(d * d + 2)
        jtj = np.ascontiguousarray(self.jtj[i], dtype=np.float64)
        _abi.check(self._lib, self._lib.rsf_fit_laplace(d, self.n_obs, float(shape), float(self.ssq[i]), _dp(jtj), _dp(_vec(lo, d, "lo")),
                                                        _dp(_vec(hi, d, "hi")), _dp(out)))
        return i, out[:d * d].reshape(d, d).copy(), float(out[d * d]), float(out[d * d + 1])

    def covariance(self, i=None):
        """rsf_fit_laplace's cov = ssq / (n_obs - d) (X^T X)^-1 of start i (by default best()) → (d, d); the standard errors are
        the square roots of its diagonal."""
        return self._laplace(1.0, 0.0, 1.0, i)[1]

    def laplace(self, shape=None, lo=0.0, hi=1.0e4, i=None):
        """rsf_fit_laplace at start i (by default best()) → dict(index, q, ssq, cov, stderr, log_integral, log_evidence, shape):
        Laplace's approximation of the integral of SSq^-shape (shape defaults to n_obs / 2) and log p(y | M) with the constants of
        Engine.evidence_finish and Engine.smc over the box (lo, hi).  The value IGNORES THE BOX'S EDGES: it is meaningful at d = 1
        with an interior mode, not on the ridge of d = 3."""
        shape = 0.5 * self.n_obs if shape is None else float(shape)
        i, cov, logi, ev = self._laplace(shape, lo, hi, i)
        return {"index": i, "q": self.q[i].copy(), "ssq": float(self.ssq[i]), "cov": cov, "stderr": np.sqrt(np.diag(cov)), "log_integral": logi,
                "log_evidence": ev, "shape": shape}


class MalaResult:
    """Result of Engine.mala / Engine.mala_from_residuals: per chain the final state q (n, d), ssq (n,), grad = X^T r (n, d) and
    jtj = X^T X (n, d, d), the counters accepted, outbox (proposals outside the box) and stuck (iterations without a proposal),
    (n,) int32, over n_iter iterations; samples (n_keep, n, d) and ssq_trace (n_keep, n), the kept states, and iterations (n_keep,),
    the 1-based iteration of each kept row.  NumPy arrays on the host.  The target is pi(q) ~ 1_box SSq^-shape; std2 completes it."""

    def __init__(self, q, ssq, grad, jtj, accepted, outbox, stuck, n_iter, samples, ssq_trace, iterations, shape, seed, offset):
        self.q, self.ssq, self.grad, self.jtj, self.accepted, self.outbox, self.stuck = q, ssq, grad, jtj, accepted, outbox, stuck
        self.n_iter, self.samples, self.ssq_trace, self.iterations = int(n_iter), samples, ssq_trace, iterations
        self.shape, self.seed, self.offset = float(shape), int(seed), int(offset)

    @property
    def accept_rate(self):
        """accepted proposals / iterations, over all chains"""
        return float(self.accepted.sum()) / (self.n_iter * self.accepted.shape[0])

    def std2(self, seed=None, engine=None, kept=False):
        """sigma^2 | q ~ InvGamma(shape, ssq / 2) by Engine.smc_std2 (l = -shape log ssq) of the final states → (n,), or with
        kept=True of the kept states → (n_keep, n), row r with the gamma variates of Philox iteration iterations[r].  seed: by
        default the run's; engine: by default a host-memory Engine made for the call."""
        seed = self.seed if seed is None else int(seed)
        rows = self.ssq_trace if kept else self.ssq[None]
        its = self.iterations if kept else [self.n_iter]
        with contextlib.nullcontext(engine) if engine is not None else Engine(mem="host") as eng:
            with np.errstate(divide="ignore", invalid="ignore"):
                out = [_host(eng.smc_std2(-self.shape * np.log(r), self.shape, seed, self.offset, int(t))) for r, t in zip(rows, its)]
        return np.stack(out) if kept else out[0]


class DrResult:
    """Result of Engine.dr / Engine.dr_from_ssq: per chain the final state q (n, d) and l = -shape log SSq (n,), the counters
    accepted1, accepted2 (proposals accepted at stage 1 and 2), outbox1, outbox2 (proposals outside the box) and stuck (iterations
    without a proposal), (n,) int32, over n_iter iterations; trace_q (n_keep, n, d) and trace_l (n_keep, n), the kept states, and
    iterations (n_keep,), the Philox iteration of each kept row; chol (G, d, d), the factor of each group in use at the end (the
    start's unless adapt_launches replaced it).  NumPy arrays on the host.  The target is pi(q) ~ 1_box SSq^-shape; std2 completes it."""

    def __init__(self, q, l, counters, n_iter, trace_q, trace_l, iterations, chol, gamma, stages, shape, seed, offset, iter0=1):
        self.q, self.l, self.iter0 = q, l, int(iter0)
        self.accepted1, self.accepted2, self.outbox1, self.outbox2, self.stuck = counters
        self.n_iter, self.trace_q, self.trace_l, self.iterations, self.chol = int(n_iter), trace_q, trace_l, iterations, chol
        self.gamma, self.stages, self.shape, self.seed, self.offset = float(gamma), int(stages), float(shape), int(seed), int(offset)

    def _rate(self, c):
        return float(c.sum()) / (self.n_iter * c.shape[0])

    @property
    def accept_rate(self):
        """iterations that moved the chain (at either stage) / iterations, over all chains"""
        return self._rate(self.accepted1) + self._rate(self.accepted2)

    @property
    def accept_rates(self):
        """(stage 1 accepted / iterations, stage 2 accepted / second proposals made)"""
        second = self.n_iter * self.q.shape[0] - int(self.stuck.sum()) - int(self.accepted1.sum())
        return self._rate(self.accepted1), (float(self.accepted2.sum()) / second if second and self.stages == 2 else 0.0)

    @property
    def outbox_rates(self):
        """(first, second) proposals outside the box / iterations, over all chains"""
        return self._rate(self.outbox1), self._rate(self.outbox2)

    @property
    def n_solves(self):
        """forward solves of the run: every first proposal inside the box, and (stages = 2) every second one inside the box"""
        c = [np.asarray(x, dtype=np.int64) for x in (self.accepted1, self.outbox1, self.outbox2, self.stuck)]
        first = int((self.n_iter - c[3] - c[1]).sum())
        return first + (int((self.n_iter - c[3] - c[0] - c[2]).sum()) if self.stages == 2 else 0)

    def std2(self, seed=None, engine=None, kept=False):
        """sigma^2 | q ~ InvGamma(shape, SSq / 2) by Engine.smc_std2 of the final states' l → (n,), or with kept=True of the kept
        states → (n_keep, n), row r with the gamma variates of Philox iteration iterations[r].  seed: by default the run's;
        engine: by default a host-memory Engine made for the call."""
        seed = self.seed if seed is None else int(seed)
        rows = self.trace_l if kept else self.l[None]
        its = self.iterations if kept else [self.iter0 + self.n_iter - 1]
        with contextlib.nullcontext(engine) if engine is not None else Engine(mem="host") as eng:
            out = [_host(eng.smc_std2(r, self.shape, seed, self.offset, int(t))) for r, t in zip(rows, its)]
        return np.stack(out) if kept else out[0]


def whole_islands(n_walkers, island_size):
    """n_walkers rounded up to whole islands of island_size walkers (the ensemble sampler runs whole islands only)"""
    n_walkers, island_size = int(n_walkers), int(island_size)
    if n_walkers < 1 or island_size < 2 or island_size % 2:
        raise ValueError("n_walkers >= 1 and an even island_size >= 2")
    return -(-n_walkers // island_size) * island_size


class EnsembleResult:
    """Result of Engine.ensemble / Engine.ensemble_from_ssq: per walker the final state q (n, d) and l = -shape log SSq (n,), the
    counters accepted, outbox (proposals outside the box) and stuck (half-steps without a proposal), (n,) int32, over n_iter
    iterations; trace_q (n_keep, n, d) and trace_l (n_keep, n), the kept states, and iterations (n_keep,), the 1-based iteration of
    each kept row.  island_size = 2 x the engine's workgroup size: walkers k island_size .. (k + 1) island_size - 1 are island k, an
    independent replicate, so Engine.diagnostics(trace_q, superchain_size=island_size) is the nested R-hat over islands.  NumPy
    arrays on the host.  The target is pi(q) ~ 1_box SSq^-shape; std2 completes it."""

    def __init__(self, q, l, accepted, outbox, stuck, n_iter, trace_q, trace_l, iterations, island_size, shape, seed, offset, logmask, a):
        self.q, self.l, self.accepted, self.outbox, self.stuck = q, l, accepted, outbox, stuck
        self.n_iter, self.trace_q, self.trace_l, self.iterations = int(n_iter), trace_q, trace_l, iterations
        self.island_size, self.shape, self.seed, self.offset, self.logmask, self.a = int(island_size), float(shape), int(seed), int(offset), int(logmask), float(a)

    @property
    def n_islands(self):
        return self.q.shape[0] // self.island_size

    @property
    def accept_rate(self):
        """accepted proposals / iterations, over all walkers"""
        return float(self.accepted.sum()) / (self.n_iter * self.accepted.shape[0])

    @property
    def outbox_rate(self):
        """proposals outside the box / iterations, over all walkers"""
        return float(self.outbox.sum()) / (self.n_iter * self.outbox.shape[0])

    def std2(self, seed=None, engine=None, kept=False):
        """sigma^2 | q ~ InvGamma(shape, SSq / 2) by Engine.smc_std2 of the final states' l → (n,), or with kept=True of the kept
        states → (n_keep, n), row r with the gamma variates of Philox iteration iterations[r].  seed: by default the run's;
        engine: by default a host-memory Engine made for the call."""
        seed = self.seed if seed is None else int(seed)
        rows = self.trace_l if kept else self.l[None]
        its = self.iterations if kept else [self.n_iter]
        with contextlib.nullcontext(engine) if engine is not None else Engine(mem="host") as eng:
            out = [_host(eng.smc_std2(r, self.shape, seed, self.offset, int(t))) for r, t in zip(rows, its)]
        return np.stack(out) if kept else out[0]


def _simpson_axis(lo, hi, n):
    """n (odd) uniform nodes on [lo, hi] and their composite Simpson weights"""
    x = np.linspace(lo, hi, n)
    w = np.full(n, 2.0)
    w[1::2] = 4.0
    w[0] = w[-1] = 1.0
    return x, w * ((hi - lo) / (n - 1) / 3.0)


def _node_cdf(x, f):
    """The CDF at the nodes x of the node density f → (density, cdf), both normalised by the integral.  Uniform nodes (four or
    more): a cell integrates the cubic through the four nearest nodes (fourth order, as the Simpson rule that weighs them); else
    the trapezoid rule."""
    h = np.diff(x)
    if x.size >= 4 and np.allclose(h, h[0], rtol=1e-9, atol=0.0):
        c = np.empty(x.size - 1)
        c[1:-1] = (-f[:-3] + 13.0 * f[1:-2] + 13.0 * f[2:-1] - f[3:]) / 24.0
        c[0] = (9.0 * f[0] + 19.0 * f[1] - 5.0 * f[2] + f[3]) / 24.0
        c[-1] = (9.0 * f[-1] + 19.0 * f[-2] - 5.0 * f[-3] + f[-4]) / 24.0
        c *= h[0]
    else:
        c = 0.5 * (f[:-1] + f[1:]) * h
    F = np.maximum.accumulate(np.concatenate([[0.0], np.cumsum(c)]))
    return f / F[-1], F / F[-1]


def _invert_cdf(x, f, F, probs, sub=16):
    """quantiles of the CDF F with the density f at the nodes x: the cubic Hermite interpolant of (F, f), tabulated on `sub` points
    per cell and inverted linearly"""
    t = (np.arange(sub) / sub)[None, :]
    h, F0, F1, f0, f1 = np.diff(x)[:, None], F[:-1, None], F[1:, None], f[:-1, None], f[1:, None]
    Fd = (2 * t ** 3 - 3 * t ** 2 + 1) * F0 + (t ** 3 - 2 * t ** 2 + t) * h * f0 + (3 * t ** 2 - 2 * t ** 3) * F1 + (t ** 3 - t ** 2) * h * f1
    xd = np.concatenate([(x[:-1, None] + t * h).ravel(), x[-1:]])
    Fd = np.maximum.accumulate(np.concatenate([Fd.ravel(), F[-1:]]))
    return np.interp(np.asarray(probs, dtype=np.float64), Fd, xd)


def _draws_pool(res, n, seed):
    """What GridPosterior.pool and LawGridPosterior.pool share: n draws of `res` as a PosteriorPool, (16, n / 16, d) when 16 divides n"""
    if __package__:
        from .MCMC import PosteriorPool
    else:
        from MCMC import PosteriorPool
    q, std2 = res.draw(n, seed)
    rows = 16 if q.shape[0] % 16 == 0 else 1
    stats = {"log_integral": res.log_integral, "log_evidence": res.log_evidence, "n_solves": res.n_solves + q.shape[0], "shape": res.shape}
    return PosteriorPool(np.ascontiguousarray(q.reshape(-1, rows, res.d).transpose(1, 0, 2)), np.ascontiguousarray(std2.reshape(-1, rows).T), 1.0, stats, 0)


class GridPosterior:
    """Result of Engine.grid_posterior / Engine.grid_from_ssq: the posterior pi(q) ~ 1_box SSq^-shape tabulated on a tensor grid —
    no Monte Carlo error.  x, w: the axes' nodes and weights; coords: 0 plain, 1 product (axis 0 is Dc a).  log_integral = log of
    the integral of SSq^-shape over the box, log_evidence with the constants of Engine.evidence_finish (comparable with
    Engine.evidence's and Engine.smc's as it stands); mean (d,) and cov (d, d) of q; std2_mean, std2_var of sigma^2's marginal;
    x0_mean, x0_var of axis 0 (Dc a in product coordinates); n_neginf nodes without density (outside the box, or a non-finite
    SSq); outside: the coarse scan's mass beyond the fine window; n_solves forward solves spent; lmax, fields, m0, cum0 and
    finish (pair, mass1, mass2, cum1, cum2): the tables.  It holds the engine that made it, which serves draw, marginal('Dc') in
    product coordinates and pool."""

    def __init__(self, engine, x, w, coords, lo, hi, shape, col, fin, ltarget, outside, n_solves):
        self.engine, self.x, self.w, self.coords, self.lo, self.hi, self.shape = engine, x, w, coords, lo, hi, shape
        self.d, self.n = len(x), tuple(a.size for a in x)
        self.lmax, self.fields, self.m0, self.cum0, self.finish = col["lmax"], col["fields"], col["m0"], col["cum0"], fin
        for k in ("Z", "log_integral", "log_evidence", "n_neginf", "mean", "cov", "x0_mean", "x0_var", "std2_mean", "std2_var"):
            setattr(self, k, fin[k])
        self._ltarget, self.outside, self.n_solves = ltarget, outside, n_solves
        self.names = ("Dc",) if self.d == 1 else (("Dc", "a", "b", "Dc*a") if coords == _abi.GRID_PRODUCT else ("Dc", "a", "b")[:self.d])
        self._dc = None

    def marginal(self, name):
        """→ (x, density, cdf) of 'Dc', 'a', 'b' or (product coordinates) 'Dc*a' on that quantity's nodes: the node density from the
        node masses, the CDF its integral (fourth order on uniform nodes, else the trapezoid rule).  'Dc' in product coordinates:
        on 4001 points over mean +- 12 SD inside the box, the CDF from dc_cdf (rsf_grid_cdf) and the density its slope."""
        if name not in self.names:
            raise ValueError(f"marginal is one of {self.names}")
        axis = {"Dc": 0, "Dc*a": 0, "a": 1, "b": 2}[name]
        if name == "Dc" and self.coords == _abi.GRID_PRODUCT:
            if self._dc is None:
                sd = math.sqrt(self.cov[0, 0])
                xs = np.linspace(max(self.lo[0], self.mean[0] - 12.0 * sd), min(self.hi[0], self.mean[0] + 12.0 * sd), 4001)
                F = self.dc_cdf(xs)
                self._dc = (xs, np.gradient(F, xs), F)
            return self._dc
        x = self.x[axis]
        f = self.m0 / self.Z if axis == 0 else self.finish[f"mass{axis}"] / self.w[axis]
        return (x,) + _node_cdf(x, f)

    def dc_cdf(self, xs, sub=4):
        """Product coordinates: the CDF of Dc at the points xs by rsf_grid_cdf, F(x) = sum over the columns of mass(c) F0(x a | c).
        As a function of a, F0(x a | a, b) is a step about as wide as the posterior of Dc a is narrow, which the nodes of the a axis
        need not resolve (at 65 nodes Dc's upper credible limit was 0.32 Monte-Carlo SE of a 262 144-draw pool off)
        although every column is resolved along Dc a and changes slowly with a.  So on a uniform a axis of four or more nodes the
        sum is taken on that axis refined `sub` times (even): the columns' CDFs at fixed Dc a and the node density of the column masses
        interpolated by the cubic through the four nearest a nodes (linear interpolation of the CDFs costs 0.1 SE on the closed form), Simpson weights on the
        refined nodes, in slabs of axis-2 nodes whose sums add.  Other axes, and sub = 1: the grid as it is."""
        eng, (x0, x1, x2), pair = self.engine, self.x, self.finish["pair"]
        n0, n1, n2 = self.n
        h = np.diff(x1)
        if int(sub) < 2 or int(sub) % 2 or n1 < 4 or not np.allclose(h, h[0], rtol=1e-9, atol=0.0):
            return eng.grid_cdf(self.x, self.cum0, pair, xs, self.coords)
        sub = int(sub)
        t = np.arange(sub) / sub
        k = np.repeat(np.arange(n1 - 1), sub)                  # the cell of each refined node but the last, and its place in it
        tt = np.tile(t, n1 - 1)
        x1r, w1r = _simpson_axis(x1[0], x1[-1], (n1 - 1) * sub + 1)
        # the node density of the masses along a: the cubic through the four nearest nodes (stencil s .. s + 3)
        st = np.clip(k - 1, 0, n1 - 4)
        tau = k - st + tt
        g = pair / self.w[1][None, :]
        lag = []
        for j in range(4):
            lj = np.ones_like(tau)
            for m in range(4):
                if m != j:
                    lj *= (tau - m) / (j - m)
            lag.append(lj)
        gr = np.zeros((n2, k.size + 1))
        for j in range(4):
            gr[:, :-1] += lag[j][None, :] * g[:, st + j]
        gr[:, -1] = g[:, -1]
        pr = np.maximum(gr, 0.0) * w1r[None, :]
        pr /= pr.sum()
        C = _host(self.cum0).reshape(n2, n1, n0)
        F = np.zeros(np.size(xs))
        for rows in np.array_split(np.arange(n2), max(1, n2 // 5)):
            c = C[rows]
            cr = sum(lag[j][None, :, None] * c[:, st + j] for j in range(4))
            # next to a column without mass (all 0): the cell's own two columns, or the one of them that has mass
            lo_, hi_ = c[:, k], c[:, k + 1]
            has_lo, has_hi = lo_[..., -1:] > 0, hi_[..., -1:] > 0
            whole = np.all(np.stack([c[:, st + j][..., -1:] > 0 for j in range(4)]), axis=0)
            lin = np.where(has_lo & has_hi, (1.0 - tt)[None, :, None] * lo_ + tt[None, :, None] * hi_, np.where(has_lo, lo_, hi_))
            cr = np.where(whole, np.clip(cr, 0.0, 1.0), lin)
            cr = np.concatenate([cr, c[:, -1:]], axis=1)
            F += eng.grid_cdf([x0, x1r, x2[rows]], np.ascontiguousarray(cr), pr[rows], xs, self.coords)
        return F

    def quantiles(self, name, probs=(0.025, 0.25, 0.5, 0.75, 0.975)):
        """the quantiles of marginal(name) at `probs`: the cubic Hermite interpolant of its CDF and density, inverted"""
        return _invert_cdf(*self.marginal(name), probs)

    def draw(self, n, seed=0, offset=0):
        """n independent draws (Engine.grid_draw; shards with offsets form one stream), each completed with
        sigma^2 | q ~ InvGamma(shape, SSq / 2) from one more evaluation of the target at the draws → (q (n, d), std2 (n,)) on the
        host.  An effective sample size of n from n solves."""
        q = self.engine.grid_draw(self.x, self.cum0, self.finish["cum1"], self.finish["cum2"], n, self.coords, seed, offset)
        std2 = self.engine.smc_std2(self._ltarget(q), self.shape, seed, offset, 1)
        return _host(q), _host(std2)

    def pool(self, n, seed=0):
        """n draws as a PosteriorPool, laid out as MCMC.sample_smc lays its particles out ((16, n / 16, d) when 16 divides n):
        predictive, loo, joint, corner, diagnostics and rank_diagnostics work on it unchanged.  Its stats carry log_integral,
        log_evidence, n_solves and shape."""
        return _draws_pool(self, n, seed)


class LawGridPosterior:
    """Result of Engine.law_grid_posterior: the posterior pi(q) ~ 1_box SSq^-shape of a state-law model tabulated on a tensor grid
    in the whitened coordinates z of a fit, phi = m + L z, q_perm[p] = phi_p or exp(phi_p) (include/rsf_law_grid.h) — no Monte
    Carlo error.  z, w: the axes' nodes and weights; m, L, tr, perm: the map; first = perm[0], the parameter of axis 0, of which
    marginal, quantiles and cdf speak.  log_integral: log of the integral of SSq^-shape over the box (the z-integral times
    prod L_pp); log_evidence with the constants of Engine.evidence_finish (comparable with Engine.law_evidence's and GridPosterior's
    as it stands); mean (d,), cov (d, d) of q and std2_mean of sigma^2's marginal from Engine.law_grid_moments; n_solves forward
    solves spent; windows: the half-width of each z-axis after any doubling.
    edge_mass: the largest share of any axis' marginal z-mass carried by that axis' two end nodes (edge_masses: per axis).  It is
    the ONLY evidence that the window holds the posterior: small, the density has died away where the window ends along every
    axis; it says nothing about mass that the fit's coordinates do not see (a second mode far from the fit).
    n_neginf: nodes without density — outside the box, or a non-finite SSq.  Where a box face cuts the window the composite
    Simpson rule runs over a discontinuity and its error is first order in the node spacing there: the result is then
    APPROXIMATE, n_neginf > 0 says so."""

    def __init__(self, engine, law, observable, data, z, w, gmap, lo, hi, shape, l, ssq, col, fin, mom, center, n_solves, windows):
        self._data = data
        self.engine, self.law, self.observable, self.z, self.w, self.lo, self.hi, self.shape = engine, law, observable, z, w, lo, hi, shape
        self.m, self.L, self.tr, self.perm = gmap
        self.d, self.n, self.first = len(z), tuple(a.size for a in z), int(self.perm[0])
        self.l, self.ssq, self.lmax, self.fields, self.m0, self.cum0, self.finish = l, ssq, col["lmax"], col["fields"], col["m0"], col["cum0"], fin
        d, logdet = self.d, float(np.log(np.diag(self.L)).sum())
        self.Z, self.n_neginf = fin["Z"], fin["n_neginf"]
        self.log_integral, self.log_evidence = fin["log_integral"] + logdet, fin["log_evidence"] + logdet
        t = mom
        self.moments, self.center = t, center
        m1 = t[1:4] / t[0]
        cov = np.empty((3, 3))
        for k, (p, r) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            cov[p, r] = cov[r, p] = t[4 + k] / t[0] - m1[p] * m1[r]
        self.mean, self.cov = center + m1[:d], cov[:d, :d].copy()
        self.std2_mean = 0.5 * t[10] / t[0] / (shape - 1.0)
        mass = [w[0] * self.m0 / self.Z] + [fin[f"mass{p}"] for p in range(1, d)]
        self.edge_masses = np.array([float(a[0] + a[-1]) for a in mass])
        self.edge_mass, self.mass = float(self.edge_masses.max()), mass
        self.n_solves, self.windows = int(n_solves), tuple(windows)
        self.names = ("Dc", "a", "b")[:d]

    def _q0(self, z0):
        """the `first` parameter at the axis-0 coordinates z0: monotone, L is lower-triangular"""
        phi = self.m[0] + self.L[0, 0] * np.asarray(z0, dtype=np.float64)
        return np.exp(phi) if self.tr[0] else phi

    def _z0(self, x):
        x = np.asarray(x, dtype=np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            phi = np.where(x > 0, np.log(np.where(x > 0, x, 1.0)), -np.inf) if self.tr[0] else x
        return (phi - self.m[0]) / self.L[0, 0]

    def marginal(self):
        """→ (x, density, cdf) of the `first` parameter on the nodes of axis 0 mapped to it: the CDF is the integral of the node
        density in z (GridPosterior.marginal's rule), the density that one divided by dq / dz."""
        f, F = _node_cdf(self.z[0], self.mass[0] / self.w[0])
        x = self._q0(self.z[0])
        return x, f / (self.L[0, 0] * (x if self.tr[0] else 1.0)), F

    def quantiles(self, probs=(0.025, 0.25, 0.5, 0.75, 0.975)):
        """the quantiles of the `first` parameter at `probs`: GridPosterior.quantiles' inversion in z, mapped"""
        f, F = _node_cdf(self.z[0], self.mass[0] / self.w[0])
        return self._q0(_invert_cdf(self.z[0], f, F, probs))

    def cdf(self, xs):
        """the CDF of the `first` parameter at the points xs (rsf_grid_cdf on the z-grid) → (len(xs),) on the host"""
        zs = np.clip(self._z0(np.atleast_1d(xs)), -1e300, 1e300)
        return self.engine.grid_cdf(self.z, self.cum0, self.finish["pair"], zs, _abi.GRID_PLAIN)

    def to_q(self, zd):
        """points (n, d) of z → q (n, d) in the order (Dc, a, b), on the host"""
        phi = self.m[None, :] + _host(zd).reshape(-1, self.d) @ self.L.T
        q = np.empty_like(phi)
        for p in range(self.d):
            q[:, int(self.perm[p])] = np.exp(phi[:, p]) if self.tr[p] else phi[:, p]
        return q

    def draw(self, n, seed=0, offset=0):
        """n independent draws: rsf_grid_draw's draws of z mapped to q, each completed with sigma^2 | q ~ InvGamma(shape, SSq / 2)
        from one more solve at the draw (Engine.law_logtarget on points) → (q (n, d), std2 (n,)) on the host.  A draw that the
        piecewise-linear inversion places outside the box (the window cut by a face) is moved onto the face.
        THE DRAWS ARE AS EXACT AS THE NODE SPACING, not exact: rsf_grid_draw inverts piecewise-linear tables and conditions each axis
        on the nearest node of the one above.  Measured by bridge sampling on 16 384 draws: at 0.25 SD between the nodes
        of every axis (the default, 65 nodes on +- 8) the pool's evidence lay 4e-4 from the grid's, within its error; at 0.5 SD on
        two axes it lay 3e-3 off, four of its standard errors.  The moments, the marginal and log_evidence do not pass through draws."""
        eng = self.engine
        zd = eng.grid_draw(self.z, self.cum0, self.finish["cum1"], self.finish["cum2"], n, _abi.GRID_PLAIN, seed, offset)
        q = np.clip(self.to_q(zd), self.lo, self.hi)
        l = eng.law_logtarget(self.law, self.observable, self._data, self.lo, self.hi, theta=q, shape=self.shape)[0]
        return q, _host(eng.smc_std2(l, self.shape, seed, offset, 1))

    def pool(self, n, seed=0):
        """n draws as a PosteriorPool, GridPosterior.pool's layout and stats: law_predictive, law_loo, joint, corner and the
        diagnostics work on it unchanged.  The pool is the posterior as well as the nodes resolve it (see draw)."""
        return _draws_pool(self, n, seed)


class Engine:
    def __init__(self, lib=None, mem="host", device=-1, block_threads=0, cpu_threads=0, stream=None, checker=False):
        if lib is None:
            lib = _abi.load()
            _abi.require_device(lib)
        elif lib.rsf_backend() != b"hip-gfx950" and not checker and os.environ.get("RSF_ALLOW_CHECKER_ENGINE") != "1":
            # `lib` exists so that the test-suite can drive the CPU oracle through this very class; nothing in the product may
            # end up on it by accident: a non-HIP library is refused unless THIS CALL declares itself a checker
            # (checker=True: __graft_entry__.smoke(), bench.py's cpu_baseline leg, tools/) — the environment variable is
            # the test-suite's process-wide form of the same declaration (tests/conftest.py) and is set nowhere else
            raise _abi.RsfError(-2, f"Engine(lib=...) was handed the {lib.rsf_backend().decode()!r} library: the product runs on "
                                    "csrc/librsf_hip.so only (no CPU fallback); a checker passes checker=True")
        self.lib = lib
        self.mem = mem
        self.device = device
        self._torch = None
        cfg = _abi.Config()
        cfg.size, cfg.version = ctypes.sizeof(_abi.Config), _abi.ABI_VERSION
        cfg.device = device
        cfg.mem_space = _abi.MEM_DEVICE if mem == "device" else _abi.MEM_HOST
        cfg.block_threads, cfg.cpu_threads = block_threads, cpu_threads
        self.block_threads = int(block_threads) or _abi.MAX_BLOCK
        if mem == "device":
            import torch

            self._torch = torch
            if device < 0:
                device = torch.cuda.current_device()
            self.device = cfg.device = device  # buffers and launches of this engine stay on this GPU whatever is current
            if stream is None:
                stream = torch.cuda.current_stream(device).cuda_stream
        cfg.stream = stream
        self._ctx = ctypes.c_void_p()
        _abi.check(lib, lib.rsf_create(ctypes.byref(cfg), ctypes.byref(self._ctx)))
        self.nout = None
        self.state_law = "aging"  # the model's (set_model)
        self.observable = "acc"   # the model's (set_model)
        self.stiffness = None     # the model's (set_model): None, the reference's coupling k' = 0.1 / Dc, or the apparatus's
        self.n_chains = self.n_params = None
        self.world = self.rank = 0  # set by comm_init

    # -- lifetime -------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_ctx", None):
            self.lib.rsf_destroy(self._ctx)
            self._ctx = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def sync(self):
        _abi.check(self.lib, self.lib.rsf_sync(self._ctx))

    # -- buffers --------------------------------------------------------------------------
    def _empty(self, shape, dtype=np.float64):
        if self.mem == "device":
            t = self._torch
            return t.empty(shape, dtype=t.uint8 if dtype == np.uint8 else t.float64, device=f"cuda:{self.device}")
        return np.empty(shape, dtype=dtype)

    def _in(self, x, dtype=np.float64):
        """Contiguous array in this engine's memory space (None passes through)."""
        if x is None:
            return None
        if self.mem == "device":
            t = self._torch
            if not isinstance(x, t.Tensor):
                x = t.as_tensor(np.ascontiguousarray(x, dtype=dtype))
            return x.to(device=f"cuda:{self.device}", dtype=t.float64).contiguous()
        return np.ascontiguousarray(x, dtype=dtype)

    @staticmethod
    def _ptr(x):
        if x is None:
            return None
        if isinstance(x, np.ndarray):
            return x.ctypes.data
        return x.data_ptr()

    # -- forward model --------------------------------------------------------------------
    def set_model(self, model, substeps=1):
        """rsf_set_model, then the model's own loading history (model.loading, if it has one: set_loading).  model.state_law
        is kept as self.state_law: the kernels of every family integrate the ageing law, so with 'slip' only law_forward and
        the calls built on it run (_need_model).  model.observable is kept as self.observable in the same way: the kernels of
        every family fit the acceleration, so with another observable only law_observe and the calls that take an ssq_fn run.
        model.stiffness is kept as self.stiffness: only the kernels of include/rsf_stiff.h carry a stiffness independent of Dc, so
        with one only law_observe, the law_dr calls and the calls that take an ssq_fn or residuals run (they route to stiff_*)."""
        law = check_law_options(model)
        observable = observable_of(model)
        stiffness = stiffness_of(model)
        m = _model_struct(model, substeps)
        _abi.check(self.lib, self.lib.rsf_set_model(self._ctx, ctypes.byref(m)))
        n = ctypes.c_int32()
        _abi.check(self.lib, self.lib.rsf_model_nout(self._ctx, ctypes.byref(n)))
        self.nout = n.value
        self.model_args = (model, substeps)
        self.state_law = law
        self.observable = observable
        self.stiffness = stiffness
        self.n_chains = self.n_params = None  # a new model invalidates the chains (rsf_abi.h: rsf_set_model)
        if getattr(model, "loading", None) is not None:
            try:
                self.set_loading(model.loading)
            except BaseException:
                self.nout = None  # no model rather than this one under the built-in history: every call asks for set_model again
                raise
        return self.nout

    def _need_model(self, law_aware=False, stiff_aware=False):
        if self.nout is None:
            raise _abi.RsfError(-3, "call set_model first")
        if not stiff_aware and getattr(self, "stiffness", None) is not None:
            raise NotImplementedError(f"this call cannot run a model with stiffness={self.stiffness!r}: {_COUPLED}, the reference's spring; a "
                                      "stiffness independent of Dc runs through law_observe, law_dr and the calls that take an ssq_fn or "
                                      "residuals")
        if not law_aware and getattr(self, "state_law", "aging") != "aging":
            raise NotImplementedError(f"this call integrates the ageing law only, and the model's state_law is {self.state_law!r}: "
                                      "the slip law runs through law_forward and the calls that take an ssq_fn; the predictive checks under a law are "
                                      "law_predictive's")
        if not law_aware and getattr(self, "observable", "acc") != "acc":
            raise NotImplementedError(f"this call fits the acceleration only, and the model's observable is {self.observable!r}: "
                                      "another observable runs through law_observe and the calls that take an ssq_fn; the predictive checks of an "
                                      "observable are law_predictive's")

    # -- the loading history and the state law (include/rsf_law.h) ---------------------------------------
    def _law_fn(self, name):
        """a function of include/rsf_law.h, which librsf_hip.so alone exports"""
        try:
            return getattr(self.lib, name)
        except AttributeError:
            raise _abi.RsfError(-5, f"{name} is exported by librsf_hip.so only: the {self.lib.rsf_backend().decode()!r} library has no such "
                                    "symbol (include/rsf_law.h)") from None

    def loading_size(self):
        """the loading table's length, 2 substeps (nout - 1) + 1"""
        self._need_model(law_aware=True, stiff_aware=True)
        n = ctypes.c_int64()
        _abi.check(self.lib, self._law_fn("rsf_loading_size")(self._ctx, ctypes.byref(n)))
        return n.value

    def loading_times(self):
        """the RK4 stage times t_start + j (delta_t / substeps) / 2 of the loading table, as rsf_set_model forms them"""
        self._need_model(law_aware=True, stiff_aware=True)
        model, substeps = self.model_args
        hh = 0.5 * (((float(model.t_final) - float(model.t_start)) / int(model.num_tsteps)) / int(substeps))
        return float(model.t_start) + np.arange(2 * int(substeps) * (self.nout - 1) + 1, dtype=np.float64) * hh

    def set_loading(self, values):
        """rsf_set_loading: the loading history V_l of every float64 RK4 solve from here on, until the next set_model.  values: an
        array of loading_size() values at loading_times(), a callable t -> V_l (called once with loading_times()), or None for the
        built-in history.  The chains of an earlier mcmc_init are discarded."""
        self._need_model(law_aware=True, stiff_aware=True)
        v = None
        if values is not None:
            t = self.loading_times()
            v = values(t) if callable(values) else values
            v = np.ascontiguousarray(np.asarray(v.cpu() if hasattr(v, "cpu") else v, dtype=np.float64))
            if v.shape != t.shape:
                raise ValueError(f"the loading history has shape {v.shape}: one value per RK4 stage time, {t.shape} (loading_times())")
            if not np.isfinite(v).all():
                raise ValueError("the loading history holds a value that is not finite")
        _abi.check(self.lib, self._law_fn("rsf_set_loading")(self._ctx, None if v is None else _dp(v), 0 if v is None else v.size))
        self.n_chains = self.n_params = None

    def loading(self):
        """rsf_get_loading: the loading table in use → (loading_size(),) on the host"""
        v = np.empty(self.loading_size())
        _abi.check(self.lib, self._law_fn("rsf_get_loading")(self._ctx, _dp(v), v.size))
        return v

    def law_forward(self, law, dc, a=None, b=None, data=None, want_ssq=False, want_acc=True):
        """rsf_law_forward: forward's arguments and results, → (ssq[C] | None, acc[nout, C] | None), under the state law `law`
        ('aging', 'ageing' or 'slip'; an integer goes to the library as it is) and the loading table in use, by the plain float64
        RK4 with a full evaluation at every stage."""
        self._need_model(law_aware=True)
        if isinstance(law, str):
            if law not in _abi.LAWS:
                raise ValueError(f"law is 'aging' (or 'ageing') or 'slip', not {law!r}")
            law = _abi.LAWS[law]
        dc = self._in(np.atleast_1d(dc) if not hasattr(dc, "data_ptr") else dc)
        C = int(dc.shape[0])
        a, b, data = self._in(a), self._in(b), self._in(data)
        if want_ssq and data is None:
            raise ValueError("want_ssq needs data")
        if data is not None and int(data.shape[0]) != self.nout:
            raise ValueError(f"data has {int(data.shape[0])} entries, the model produces {self.nout}")
        ssq = self._empty((C,)) if want_ssq else None
        acc = self._empty((self.nout, C)) if want_acc else None
        _abi.check(self.lib, self._law_fn("rsf_law_forward")(self._ctx, int(law), C, self._ptr(dc), self._ptr(a), self._ptr(b), self._ptr(data), self._ptr(ssq), self._ptr(acc)))
        return ssq, acc

    # -- the observable of the state-law solve (include/rsf_observe.h) -----------------------------------
    def _observe_fn(self, name):
        """a function of include/rsf_observe.h, which librsf_hip.so alone exports"""
        try:
            return getattr(self.lib, name)
        except AttributeError:
            raise _abi.RsfError(-5, f"{name} is exported by librsf_hip.so only: the {self.lib.rsf_backend().decode()!r} library has no such "
                                    "symbol (include/rsf_observe.h)") from None

    def _stiff_fn(self, name):
        """a function of include/rsf_stiff.h, which librsf_hip.so alone exports"""
        try:
            return getattr(self.lib, name)
        except AttributeError:
            raise _abi.RsfError(-5, f"{name} is exported by librsf_hip.so only: the {self.lib.rsf_backend().decode()!r} library has no such "
                                    "symbol (include/rsf_stiff.h)") from None

    def _stiffness(self, stiffness):
        """the stiffness in force for a call: the keyword's, or (None) the engine's model's → a float, or None for the coupling"""
        k = getattr(self, "stiffness", None) if stiffness is None else stiffness
        return None if k is None else float(k)

    def stiff_observe(self, law, observable, stiffness, dc, a=None, b=None, data=None, want_ssq=False, want_series=True):
        """rsf_stiff_observe: law_observe — its arguments, checks and results — with the spring's stiffness `stiffness`, a constant
        independent of Dc (include/rsf_stiff.h), in place of the reference's coupling k' = 0.1 / Dc."""
        return self.law_observe(law, observable, dc, a=a, b=b, data=data, want_ssq=want_ssq, want_series=want_series, stiffness=float(stiffness))

    def law_observe(self, law, observable, dc, a=None, b=None, data=None, want_ssq=False, want_series=True, stiffness=None):
        """rsf_law_observe: law_forward's solve, arguments and checks, → (ssq[C] | None, series[nout, C] | None) of `observable`:
        'acc' (law_forward's results, bit for bit), 'mu' (or 'friction'), 'theta' (or 'state'), 'velocity' (or 'V'); an integer
        goes to the library as it is.  data is a series of the same observable.  stiffness: None, the engine's model's; with one
        in force the call is rsf_stiff_observe."""
        self._need_model(law_aware=True, stiff_aware=True)
        k = self._stiffness(stiffness)
        if isinstance(law, str):
            if law not in _abi.LAWS:
                raise ValueError(f"law is 'aging' (or 'ageing') or 'slip', not {law!r}")
            law = _abi.LAWS[law]
        if isinstance(observable, str):
            observable = _abi.OBSERVABLES[observable_name(observable)]
        dc = self._in(np.atleast_1d(dc) if not hasattr(dc, "data_ptr") else dc)
        C = int(dc.shape[0])
        a, b, data = self._in(a), self._in(b), self._in(data)
        if want_ssq and data is None:
            raise ValueError("want_ssq needs data")
        if data is not None and int(data.shape[0]) != self.nout:
            raise ValueError(f"data has {int(data.shape[0])} entries, the model produces {self.nout}")
        ssq = self._empty((C,)) if want_ssq else None
        series = self._empty((self.nout, C)) if want_series else None
        if k is not None:
            _abi.check(self.lib, self._stiff_fn("rsf_stiff_observe")(self._ctx, int(law), int(observable), k, C, self._ptr(dc), self._ptr(a),
                                                                     self._ptr(b), self._ptr(data), self._ptr(ssq), self._ptr(series)))
            return ssq, series
        _abi.check(self.lib, self._observe_fn("rsf_law_observe")(self._ctx, int(law), int(observable), C, self._ptr(dc), self._ptr(a), self._ptr(b),
                                                                 self._ptr(data), self._ptr(ssq), self._ptr(series)))
        return ssq, series

    def law_ssq_fn(self, law, data, observable="acc", stiffness=None):
        """The ssq_fn of smc_from_ssq, dr_from_ssq, grid_from_ssq and grid_posterior for the device model under `law`: points
        (m, 1) of Dc or (m, 3) of (Dc, a, b) on the host → SSq (m,) on the host, solved by law_forward — or, with `data` a series
        of another observable than 'acc' or with a stiffness in force (stiffness: None, the engine's model's), by law_observe."""
        obs = self._in(data)
        k = self._stiffness(stiffness)
        if observable_name(observable) == "acc" and k is None:
            solve = lambda dc, a, b: self.law_forward(law, dc, a, b, data=obs, want_ssq=True, want_acc=False)[0]
        else:
            solve = lambda dc, a, b: self.law_observe(law, observable, dc, a, b, data=obs, want_ssq=True, want_series=False, stiffness=k)[0]

        def ssq_fn(pts):
            pts = np.asarray(pts, dtype=np.float64)
            pts = pts.reshape(-1, 1) if pts.ndim < 2 else pts
            ab = [np.ascontiguousarray(pts[:, p]) for p in (1, 2)] if pts.shape[1] == 3 else [None, None]
            return _host(solve(np.ascontiguousarray(pts[:, 0]), ab[0], ab[1]))

        return ssq_fn

    def _need_chains(self):
        if self.n_chains is None:
            raise _abi.RsfError(-3, "call mcmc_init first")

    def forward(self, dc, a=None, b=None, data=None, want_ssq=False, want_acc=True):
        """→ (ssq[C] | None, acc[nout, C] | None) for C parameter sets."""
        self._need_model()
        dc = self._in(np.atleast_1d(dc) if not hasattr(dc, "data_ptr") else dc)
        C = int(dc.shape[0])
        a, b, data = self._in(a), self._in(b), self._in(data)
        if want_ssq and data is None:
            raise ValueError("want_ssq needs data")
        if data is not None and int(data.shape[0]) != self.nout:
            raise ValueError(f"data has {int(data.shape[0])} entries, the model produces {self.nout}")
        ssq = self._empty((C,)) if want_ssq else None
        acc = self._empty((self.nout, C)) if want_acc else None
        _abi.check(self.lib, self.lib.rsf_forward_batch(self._ctx, C, self._ptr(dc), self._ptr(a), self._ptr(b),
                                                        self._ptr(data), self._ptr(ssq), self._ptr(acc)))
        return ssq, acc

    # -- sampler --------------------------------------------------------------------------
    def mcmc_init(self, q0, data, lo, hi, seed=0, chain_offset=0, n0=0.01, prior_len=0, adapt_mode="none",
                  adapt_interval=10, fd_rel_step=1e-6):
        self._need_model()
        q0 = self._in(q0)
        if q0.ndim == 1:
            q0 = q0.reshape(-1, 1)
        C, d = int(q0.shape[0]), int(q0.shape[1])
        data = self._in(data)
        n_groups = int(data.shape[0]) if data.ndim == 2 else 1  # (G, nout): one observation series per chain group
        if int(data.shape[-1]) != self.nout:
            raise ValueError(f"data has {int(data.shape[-1])} entries per series, the model produces {self.nout}")
        if C % n_groups:
            raise ValueError(f"{C} chains cannot be split evenly over {n_groups} observation groups")
        cfg = self._mcmc_config(C, d, lo, hi, seed, chain_offset, n0, prior_len, adapt_mode, adapt_interval, fd_rel_step, n_groups)
        _abi.check(self.lib, self.lib.rsf_mcmc_init(self._ctx, ctypes.byref(cfg), self._ptr(q0), self._ptr(data)))
        self.n_chains, self.n_params = C, d

    def _mcmc_config(self, C, d, lo, hi, seed=0, chain_offset=0, n0=0.01, prior_len=0, adapt_mode="none", adapt_interval=10,
                     fd_rel_step=1e-6, n_groups=1):
        lo, hi = _vec(lo, d, "lo"), _vec(hi, d, "hi")
        cfg = _abi.McmcConfig()
        cfg.size = ctypes.sizeof(_abi.McmcConfig)
        cfg.n_params, cfg.n_chains, cfg.chain_offset = d, C, int(chain_offset)
        cfg.seed, cfg.n0, cfg.prior_len = int(seed), float(n0), int(prior_len)
        cfg.adapt_mode = _abi.ADAPT_MODES[adapt_mode] if isinstance(adapt_mode, str) else int(adapt_mode)
        cfg.adapt_interval, cfg.fd_rel_step, cfg.n_groups = int(adapt_interval), float(fd_rel_step), n_groups
        for p in range(d):
            cfg.lo[p], cfg.hi[p] = float(lo[p]), float(hi[p])
        return cfg

    def mcmc_init_state(self, q, ssq, std2, V, lo, hi, **kw):
        """Chains from an explicit state (rsf_mcmc_init_state): no model, no observation — the sampler as an operator over
        a likelihood the caller evaluates; advanced by mcmc_replay_ssq only.  q (C, d), ssq (C,), std2 (C,), V (C, d, d)."""
        q = self._in(q)
        if q.ndim == 1:
            q = q.reshape(-1, 1)
        C, d = int(q.shape[0]), int(q.shape[1])
        ssq, std2, V = self._in(ssq), self._in(std2), self._in(V)
        if int(np.prod(ssq.shape)) != C or int(np.prod(std2.shape)) != C or int(np.prod(V.shape)) != C * d * d:
            raise ValueError("ssq and std2 hold one value per chain, V one (d, d) matrix per chain")
        cfg = self._mcmc_config(C, d, lo, hi, **kw)
        _abi.check(self.lib, self.lib.rsf_mcmc_init_state(self._ctx, ctypes.byref(cfg), self._ptr(q), self._ptr(ssq), self._ptr(std2),
                                                          self._ptr(V)))
        self.n_chains, self.n_params = C, d

    def mcmc_propose(self, z):
        """The proposals the next iteration will make from the normals z (C, d) → (q_new (C, d), in_bounds (C,) uint8)."""
        self._need_chains()
        C, d = self.n_chains, self.n_params
        z = self._in(z)
        if int(np.prod(z.shape)) != C * d:
            raise ValueError(f"z must hold {d} normals for each of the {C} chains")
        qn, inb = self._empty((C, d)), self._empty((C,), np.uint8)
        _abi.check(self.lib, self.lib.rsf_mcmc_propose(self._ctx, self._ptr(z), self._ptr(qn), self._ptr(inb)))
        return qn, inb

    def _replay_args(self, z, u, g, ssq_new=None):
        """The variates of n = u.shape[0] iterations in this engine's memory space, each of the size the library reads."""
        self._need_chains()
        C, d = self.n_chains, self.n_params
        z, u, g, ssq_new = self._in(z), self._in(u), self._in(g), self._in(ssq_new)
        n = int(u.shape[0])
        for name, x, per in (("z", z, C * d), ("u", u, C), ("g", g, C), ("ssq_new", ssq_new, C)):
            if x is not None and math.prod(x.shape) != n * per:
                raise ValueError(f"{name} holds {math.prod(x.shape)} values, not the {n * per} of {n} iterations (u.shape[0]) of {C} chains")
        return n, z, u, g, ssq_new

    def mcmc_replay_ssq(self, z, u, g, ssq_new, traces=True):
        """mcmc_replay with the proposals' sums of squares supplied by the caller (n, C): the chain logic alone."""
        n_iters, z, u, g, ssq_new = self._replay_args(z, u, g, ssq_new)
        tq, ts, ta = self._traces(n_iters, traces)
        _abi.check(self.lib, self.lib.rsf_mcmc_replay_ssq(self._ctx, n_iters, self._ptr(z), self._ptr(u), self._ptr(g), self._ptr(ssq_new),
                                                          self._ptr(tq), self._ptr(ts), self._ptr(ta)))
        return tq, ts, ta

    def get_state(self):
        self._need_chains()
        C, d = self.n_chains, self.n_params
        q, ssq, std2, V = self._empty((C, d)), self._empty((C,)), self._empty((C,)), self._empty((C, d, d))
        _abi.check(self.lib, self.lib.rsf_mcmc_get_state(self._ctx, self._ptr(q), self._ptr(ssq), self._ptr(std2), self._ptr(V)))
        return q, ssq, std2, V

    def set_state(self, q=None, ssq=None, std2=None, V=None):
        q, ssq, std2, V = self._in(q), self._in(ssq), self._in(std2), self._in(V)
        _abi.check(self.lib, self.lib.rsf_mcmc_set_state(self._ctx, self._ptr(q), self._ptr(ssq), self._ptr(std2), self._ptr(V)))

    def _traces(self, n_iters, want):
        self._need_chains()
        C, d = self.n_chains, self.n_params
        if want is True:
            want = ("q", "std2", "accept")
        want = want or ()
        tq = self._empty((n_iters, C, d)) if "q" in want else None
        ts = self._empty((n_iters, C)) if "std2" in want else None
        ta = self._empty((n_iters, C), np.uint8) if "accept" in want else None
        return tq, ts, ta

    def mcmc_run(self, n_iters, traces=True, out=None):
        """n_iters fused iterations for every chain → (trace_q[n,C,d], trace_std2[n,C], accept[n,C])."""
        tq, ts, ta = out if out is not None else self._traces(n_iters, traces)
        _abi.check(self.lib, self.lib.rsf_mcmc_run(self._ctx, int(n_iters), self._ptr(tq), self._ptr(ts), self._ptr(ta)))
        return tq, ts, ta

    def mcmc_replay(self, z, u, g, traces=True):
        """n = u.shape[0] iterations on the caller's variates: normals z (n, C, d), uniforms u (n, C), gamma variates g (n, C)."""
        n_iters, z, u, g, _ = self._replay_args(z, u, g)
        tq, ts, ta = self._traces(n_iters, traces)
        _abi.check(self.lib, self.lib.rsf_mcmc_replay(self._ctx, n_iters, self._ptr(z), self._ptr(u), self._ptr(g),
                                                      self._ptr(tq), self._ptr(ts), self._ptr(ta)))
        return tq, ts, ta

    def stats(self):
        v = [ctypes.c_int64() for _ in range(4)]
        _abi.check(self.lib, self.lib.rsf_mcmc_stats(self._ctx, *[ctypes.byref(x) for x in v]))
        return dict(zip(("accepted", "evaluated", "nonfinite", "iters_done"), (x.value for x in v)))

    def counters(self):
        """rsf_mcmc_counters → dict: the chain totals plus, on the HIP library, how the float64 RK4 kernels spent their
        wave-steps (tier by tier, redone trips, lane utilisation); `lane_utilisation` is derived."""
        v = (ctypes.c_int64 * len(_abi.COUNTERS))()
        _abi.check(self.lib, self.lib.rsf_mcmc_counters(self._ctx, v, len(_abi.COUNTERS)))
        c = dict(zip(_abi.COUNTERS, (int(x) for x in v)))
        steps = c["steps_tight"] + c["steps_narrow"] + c["steps_wide"] + c["steps_full"]
        c["lane_utilisation"] = c["lane_steps"] / (64.0 * steps) if steps else None
        return c

    # -- posterior post-processing (RSF.plot_dist, RSF.py:717-746) -------------------------
    def _block(self, samples, param=0):
        """samples: (n,) or a trace block (..., d) in this engine's memory space, `param` one of its columns → (array, n, d)."""
        x = self._in(samples)
        d = int(x.shape[-1]) if x.ndim > 1 else 1
        if not 0 <= int(param) < d:
            raise ValueError(f"param = {param!r}: a column index in [0, {d})")
        return x, int(np.prod(x.shape)) // d, d

    def pool_summary(self, samples, param=0):
        """→ dict(n, mean, var (ddof=1), min, max) of parameter `param` over all pooled draws."""
        x, n, d = self._block(samples, param)
        out = (ctypes.c_double * 5)()
        _abi.check(self.lib, self.lib.rsf_pool_summary(self._ctx, n, self._ptr(x) + 8 * int(param), d, out))
        return dict(zip(("n", "mean", "var", "min", "max"), list(out)))

    def pool_kde(self, samples, grid, param=0, bw_factor=0.0):
        """scipy.stats.gaussian_kde(samples).pdf(grid) (Scott bandwidth unless bw_factor > 0) → density[m]."""
        x, n, d = self._block(samples, param)
        grid = self._in(grid)
        m = int(grid.shape[0])
        dens = self._empty((m,))
        _abi.check(self.lib, self.lib.rsf_pool_kde(self._ctx, n, self._ptr(x) + 8 * int(param), d, m, self._ptr(grid), float(bw_factor),
                                                   self._ptr(dens)))
        return dens

    def pool_histogram(self, samples, nbins, lo, hi, param=0):
        """numpy.histogram(samples, nbins, (lo, hi)) of parameter `param` over all pooled draws, plus the out-of-range counts:
        → counts[nbins + 2] (float64 holding exact integers): [below lo, bin 0 .. bin nbins-1, above hi or NaN].  The summary path
        of SURVEY §8e: a few KB per rank, summed across ranks with pool_allreduce_sum / dist.allreduce_histogram."""
        x, n, d = self._block(samples, param)
        counts = self._empty((int(nbins) + 2,))
        _abi.check(self.lib, self.lib.rsf_pool_histogram(self._ctx, n, self._ptr(x) + 8 * int(param), d, int(nbins), float(lo), float(hi),
                                                         self._ptr(counts)))
        return counts

    # -- the joint posterior of the pooled draws (include/rsf_joint.h) ---------------------------
    @staticmethod
    def _pair(params, d):
        pa, pb = (int(p) for p in params)
        if not (0 <= pa < d and 0 <= pb < d and pa != pb):
            raise ValueError(f"params = {tuple(params)!r}: two different column indices in [0, {d})")
        return pa, pb

    def pool_joint_partials(self, samples, center=None):
        """rsf_pool_joint_partials: the additive partials of the joint moments of all d <= JOINT_MAX_PARAMS columns of the pooled
        draws (..., d) about `center` (d,) (default: the first row, as pool_summary shifts by the first sample) →
        (JOINT_HEAD + d + d (d + 1) / 2,) float64 on the host: n_finite, nonfinite (rows with a non-finite entry, left out), the
        sums and the upper triangle of the sums of products.  Partials of shards about the same centre add
        (pool_allreduce_sum, dist.allreduce_joint_partials).  With the default centre, pass samples[0] to pool_joint_finish."""
        x, n, d = self._block(samples)
        if not 1 <= d <= _abi.JOINT_MAX_PARAMS:
            raise ValueError(f"the joint moments take 1 to {_abi.JOINT_MAX_PARAMS} columns, not {d}")
        c = _host(x.reshape(n, d)[0] if center is None else center).reshape(-1)
        if c.shape != (d,):
            raise ValueError(f"center has {c.size} entries, the draws have {d} columns")
        out = np.empty(_abi.JOINT_HEAD + d + d * (d + 1) // 2)
        _abi.check(self.lib, self.lib.rsf_pool_joint_partials(self._ctx, n, d, self._ptr(x), _dp(c), _dp(out)))
        return out

    def pool_joint_finish(self, partials, center):
        """rsf_pool_joint_finish (host only): summed partials and their centre → dict(n, nonfinite, mean (d,), cov (d, d) with
        ddof = 1 as np.cov, corr (d, d) as np.corrcoef).  Fewer than two finite rows: cov and corr are NaN; a column of zero
        variance has NaN in its row and column of corr."""
        part, c = _host(partials).reshape(-1), _host(center).reshape(-1)
        d = int(c.size)
        if part.size != _abi.JOINT_HEAD + d + d * (d + 1) // 2:
            raise ValueError(f"{part.size} partials do not belong to a centre of {d} columns")
        out = np.empty(d + 2 * d * d)
        _abi.check(self.lib, self.lib.rsf_pool_joint_finish(d, _dp(part), _dp(c), _dp(out)))
        return {"n": int(part[0]), "nonfinite": int(part[1]), "mean": out[:d].copy(), "cov": out[d:d + d * d].reshape(d, d).copy(),
                "corr": out[d + d * d:].reshape(d, d).copy()}

    def pool_joint(self, samples, center=None):
        """Mean, covariance and correlation matrix of all columns of the pooled draws (..., d) → dict(n, nonfinite, mean (d,),
        cov (d, d), corr (d, d)); see pool_joint_partials and pool_joint_finish."""
        x, n, d = self._block(samples)
        c = _host(x.reshape(n, d)[0] if center is None else center).reshape(-1)
        return self.pool_joint_finish(self.pool_joint_partials(x, c), c)

    def pool_kde2d(self, samples, points, params=(0, 1), bw_factor=0.0, cov=None, n_total=None):
        """scipy.stats.gaussian_kde(samples[:, params].T).pdf(points.T) at the m points (m, 2) (Scott bandwidth n^(-1/6) unless
        bw_factor > 0) → density[m] in this engine's memory space.  cov (2, 2) and n_total evaluate a shard of a larger pool with
        the pool's covariance and size: the results of disjoint shards then add to the density of the whole pool."""
        x, n, d = self._block(samples)
        pa, pb = self._pair(params, d)
        pts = self._in(points)
        if pts.ndim != 2 or int(pts.shape[1]) != 2 or int(pts.shape[0]) < 1:
            raise ValueError("points is (m, 2)")
        m = int(pts.shape[0])
        cv = None
        if cov is not None:
            cv = _host(cov)
            if cv.shape != (2, 2):
                raise ValueError("cov is the (2, 2) covariance of the two columns")
        dens = self._empty((m,))
        _abi.check(self.lib, self.lib.rsf_pool_kde2d(self._ctx, n, d, self._ptr(x), pa, pb, m, self._ptr(pts), float(bw_factor),
                                                     None if cv is None else _dp(cv), int(n_total or 0), self._ptr(dens)))
        return dens

    def pool_histogram2d(self, samples, nbins, ranges, params=(0, 1)):
        """numpy.histogram2d(samples[:, pa], samples[:, pb], nbins, ranges) over all pooled draws, plus the out-of-range counts:
        nbins an int or (nbx, nby), ranges ((lo_a, hi_a), (lo_b, hi_b)) → counts[nbx + 2, nby + 2] (float64 holding exact
        integers) in this engine's memory space; per axis index 0 is below lo, nb + 1 above hi or NaN, and [1:-1, 1:-1] is
        numpy's result.  (nbx + 2) (nby + 2) <= HIST2D_MAX_CELLS.  Counts of shards add (pool_allreduce_sum)."""
        x, n, d = self._block(samples)
        pa, pb = self._pair(params, d)
        nbx, nby = (int(nbins), int(nbins)) if np.ndim(nbins) == 0 else (int(b) for b in nbins)
        (lo_a, hi_a), (lo_b, hi_b) = ranges
        if nbx < 1 or nby < 1:
            raise ValueError("at least one bin on each axis")
        counts = self._empty((nbx + 2, nby + 2))
        _abi.check(self.lib, self.lib.rsf_pool_histogram2d(self._ctx, n, d, self._ptr(x), pa, pb, nbx, float(lo_a), float(hi_a), nby,
                                                           float(lo_b), float(hi_b), self._ptr(counts)))
        return counts

    def pool_hpd_levels(self, weights, probs):
        """rsf_pool_hpd_levels (host only): the contour levels of a corner plot.  weights >= 0 (histogram counts, or densities on
        a regular grid; any shape) and probabilities strictly inside (0, 1) → levels[len(probs)]: levels[k] is the largest of
        the weights w for which the weights >= w hold at least probs[k] of the total."""
        w = _host(weights).reshape(-1)
        p = _probs(probs, None, False, "probs")  # the range is the library's to refuse
        if w.size < 1:
            raise ValueError("weights and probs are non-empty")
        out = np.empty(p.size)
        _abi.check(self.lib, self.lib.rsf_pool_hpd_levels(int(w.size), _dp(w), int(p.size), _dp(p), _dp(out)))
        return out

    # -- the marginal likelihood of the pooled draws by bridge sampling (include/rsf_evidence.h) -----------
    @staticmethod
    def _ev_flags(transform, d):
        """transform: None (identity), or per parameter a truthy value / "log" for phi_p = log q_p → int32 (d,)."""
        if transform is None:
            return np.zeros(d, dtype=np.int32)
        if isinstance(transform, np.ndarray) and transform.dtype == np.int32 and transform.shape == (d,):
            return transform
        t = [1 if (x == "log" or x is True or x == 1) else 0 if (x in ("identity", None) or x is False or x == 0) else -1
             for x in (transform if np.ndim(transform) else [transform] * d)]
        if len(t) != d or -1 in t:
            raise ValueError(f"transform is None or {d} entries of 'identity' / 'log' (0 / 1)")
        return np.asarray(t, dtype=np.int32)

    @staticmethod
    def _ev_gauss(mean, chol):
        m = _host(mean).reshape(-1)
        d = int(m.size)
        L = _host(chol).reshape(-1)
        if not 1 <= d <= _abi.EVIDENCE_MAX_PARAMS or L.size != d * d:
            raise ValueError(f"mean is (d,) and chol (d, d) with 1 <= d <= {_abi.EVIDENCE_MAX_PARAMS}")
        return m, L, d

    def evidence_propose(self, mean, chol, lo, hi, n2, transform=None, seed=0, offset=0):
        """rsf_evidence_propose: n2 draws of the Gaussian proposal N(mean, chol chol^T) in the working coordinates (phi_p = q_p, or
        log q_p where transform[p] is "log") → (theta (n2, d) in natural coordinates, logg (n2,), inbox (n2,) uint8) in this
        engine's memory space.  Draw j uses the normals of draws(seed, offset + j, 0, d): shards with offsets form one stream."""
        m, L, d = self._ev_gauss(mean, chol)
        tr = self._ev_flags(transform, d)
        lo, hi = _vec(lo, d, "lo"), _vec(hi, d, "hi")
        n2 = int(n2)
        theta, logg, inbox = self._empty((max(n2, 0), d)), self._empty((max(n2, 0),)), self._empty((max(n2, 0),), np.uint8)
        _abi.check(self.lib, self.lib.rsf_evidence_propose(self._ctx, n2, d, _dp(m), _dp(L), _i32p(tr), _dp(lo), _dp(hi), int(seed),
                                                           int(offset), self._ptr(theta), self._ptr(logg), self._ptr(inbox)))
        return theta, logg, inbox

    def evidence_logg(self, theta, mean, chol, transform=None):
        """rsf_evidence_logg: log g at the points theta (n, d) (natural coordinates) → (n,) in this engine's memory space."""
        m, L, d = self._ev_gauss(mean, chol)
        tr = self._ev_flags(transform, d)
        x = self._in(theta)
        n = int(np.prod(x.shape)) // d
        if int(np.prod(x.shape)) != n * d:
            raise ValueError(f"theta is (n, {d})")
        logg = self._empty((n,))
        _abi.check(self.lib, self.lib.rsf_evidence_logg(self._ctx, n, d, self._ptr(x), _dp(m), _dp(L), _i32p(tr), self._ptr(logg)))
        return logg

    def evidence_logtarget(self, theta, data, lo, hi, logg, shape=None, transform=None):
        """rsf_evidence_logtarget, the fused hot path: one float64 RK4 solve per point theta (n,) or (n, d), d = 1 or 3, and
        l = -shape log SSq + sum of log theta_p over the logged parameters - logg → (n,) in this engine's memory space; -inf
        outside the strict box (lo, hi) and where SSq is not finite.  shape defaults to nout / 2, the sampler's at n0 = 0."""
        self._need_model()
        x, g, obs = self._in(theta), self._in(logg), self._in(data)
        if x.ndim == 1:
            x = x.reshape(-1, 1)
        n, d = int(x.shape[0]), int(x.shape[1])
        if int(np.prod(g.shape)) != n:
            raise ValueError(f"logg holds {int(np.prod(g.shape))} values, theta {n} points")
        if obs.ndim != 1 or int(obs.shape[0]) != self.nout:
            raise ValueError(f"data has shape {tuple(obs.shape)}, the model produces {self.nout} samples")
        tr = self._ev_flags(transform, d)
        lo, hi = _vec(lo, d, "lo"), _vec(hi, d, "hi")
        l = self._empty((n,))
        _abi.check(self.lib, self.lib.rsf_evidence_logtarget(self._ctx, n, d, self._ptr(x), self._ptr(obs),
                                                             float(0.5 * self.nout if shape is None else shape), _dp(lo), _dp(hi),
                                                             _i32p(tr), self._ptr(g), self._ptr(l)))
        return l

    def evidence_partials(self, l1, l2, lstar, r, s1=None, s2=None):
        """rsf_evidence_partials: the additive partials of one bridge iteration at (r, lstar) over the posterior draws' l1 and the
        proposal draws' l2 (either may be empty) → (len(EVIDENCE_PARTIALS),) float64 on the host.  s1, s2 default to
        N1 / (N1 + N2) and N2 / (N1 + N2) of these arrays; a shard of a larger pool passes the pool's, and the partials of
        disjoint shards add (pool_allreduce_sum, dist.allreduce_evidence_partials)."""
        a, b = self._in(l1), self._in(l2)
        n1, n2 = int(np.prod(a.shape)), int(np.prod(b.shape))
        if s1 is None or s2 is None:
            if n1 + n2 == 0:
                raise ValueError("both sets are empty")
            s1, s2 = n1 / (n1 + n2), n2 / (n1 + n2)
        out = np.empty(len(_abi.EVIDENCE_PARTIALS))
        _abi.check(self.lib, self.lib.rsf_evidence_partials(self._ctx, n1, self._ptr(a) if n1 else None, n2, self._ptr(b) if n2 else None,
                                                            float(lstar), float(r), float(s1), float(s2), _dp(out)))
        return out

    def evidence_finish(self, partials, r, lstar, ess_factor=1.0, shape=None, lo=None, hi=None):
        """rsf_evidence_finish (host only): summed partials taken at (r, lstar) → dict(r_next, log_integral, log_evidence, re).
        Without shape, lo and hi the constants of log_evidence are unknown and it is None."""
        part = _host(partials).reshape(-1)
        if part.size != len(_abi.EVIDENCE_PARTIALS):
            raise ValueError(f"{part.size} partials, not {len(_abi.EVIDENCE_PARTIALS)}")
        full = shape is not None and lo is not None and hi is not None
        d = int(np.size(lo)) if full else 0
        lo, hi = (_vec(lo, d, "lo"), _vec(hi, d, "hi")) if full else (None, None)
        out = np.empty(len(_abi.EVIDENCE_OUT))
        _abi.check(self.lib, self.lib.rsf_evidence_finish(_dp(part), float(r), float(lstar), float(ess_factor), float(shape) if full else 1.0,
                                                          d, _dp(lo) if full else None, _dp(hi) if full else None, _dp(out)))
        res = dict(zip(_abi.EVIDENCE_OUT, (float(v) for v in out)))
        if not full:
            res["log_evidence"] = None
        return res

    def evidence_bridge(self, l1, l2, ess_factor=1.0, lstar=None, shape=None, lo=None, hi=None, return_state=False):
        """The bridge iteration on l = log target - log proposal of the N1 posterior draws (l1) and the N2 proposal draws (l2, -inf
        for a draw outside the support), from r = 1: until |r_next - r| / r_next < EVIDENCE_RTOL, EVIDENCE_MAX_ITER iterations at
        most → dict(log_integral = log r + lstar, log_evidence (None without shape, lo, hi), re, iterations, n2_in_box (the
        finite l2), converged).  lstar defaults to the median of l1.  No proposal draw inside the support: r = 0, log_integral
        -inf, re +inf, converged False."""
        a, b = self._in(l1), self._in(l2)
        if lstar is None:
            lstar = float(np.median(_host(a)))
        r, it, conv = 1.0, 0, False
        while it < _abi.EVIDENCE_MAX_ITER:
            part = self.evidence_partials(a, b, lstar, r)
            res = self.evidence_finish(part, r, lstar, ess_factor, shape, lo, hi)
            it += 1
            rn = res["r_next"]
            if not rn > 0.0:
                r = 0.0
                break
            conv = abs(rn - r) < _abi.EVIDENCE_RTOL * rn
            r = rn
            if conv:
                break
        out = {"log_integral": res["log_integral"], "log_evidence": res["log_evidence"], "re": res["re"], "iterations": it,
               "n2_in_box": int(part[2]), "converged": bool(conv)}
        if return_state:
            out.update(r=r, lstar=lstar, partials=part)
        return out

    def _evidence(self, samples, ltarget, lo, hi, shape, n_data, transform, n_proposal, fit_fraction, seed, ess_factor):
        """What evidence and evidence_from_ssq share.  ltarget(theta (n, d), logg (n,)) → l (n,)."""
        x = self._in(samples)
        trace = x.ndim == 3
        if x.ndim == 1:
            x = x.reshape(-1, 1)
        d = int(x.shape[-1])
        rows = int(x.shape[0])  # iterations of a kept trace (n, C, d), draws of a flat pool (n, d)
        k = int(round(float(fit_fraction) * rows))
        if not 0.0 < float(fit_fraction) < 1.0 or k < d + 1 or rows - k < 1:
            raise ValueError(f"fit_fraction = {fit_fraction!r} leaves {k} rows to fit the proposal and {rows - k} for the estimator")
        tr = self._ev_flags(transform, d)
        lo, hi = _vec(lo, d, "lo"), _vec(hi, d, "hi")
        fit, est = x[:k].reshape(-1, d), x[k:].reshape(-1, d)
        n1 = int(est.shape[0])
        # the proposal's moments: pool_joint of the first part in the working coordinates
        phi = fit.clone() if hasattr(fit, "clone") else fit.copy()
        for p in np.flatnonzero(tr):
            phi[:, p] = phi[:, p].log() if hasattr(phi, "log") else np.log(phi[:, p])
        mom = self.pool_joint(phi)
        if mom["nonfinite"] or not np.isfinite(mom["cov"]).all():
            raise ValueError("the first part of the draws is not finite in the working coordinates (a logged parameter <= 0?)")
        mean, chol = mom["mean"], np.linalg.cholesky(mom["cov"])
        n2 = n1 if n_proposal is None else int(n_proposal)
        theta, logg2, _ = self.evidence_propose(mean, chol, lo, hi, n2, tr, seed=seed)
        l2 = ltarget(theta, logg2)
        l1 = ltarget(est, self.evidence_logg(est, mean, chol, tr))
        res = self.evidence_bridge(l1, l2, 1.0 if ess_factor is None else float(ess_factor), None, shape, lo, hi, return_state=True)
        r, lstar, part = res.pop("r"), res.pop("lstar"), res.pop("partials")
        if ess_factor is None and trace and r > 0.0:
            # the effective number of posterior draws, from the existing diagnostics' ESS of the series f2 = 1 / (s1 p + s2)
            s1, s2 = n1 / (n1 + n2), n2 / (n1 + n2)
            f2 = 1.0 / (s1 * np.exp(np.minimum(_host(l1) - (np.log(r) + lstar), 700.0)) + s2)
            f2 = f2.reshape(rows - k, -1)
            ess = self.diagnostics(f2)[0]["ess"] if f2.shape[0] >= 4 and f2.std() > 0 else float(n1)
            ess_factor = float(min(1.0, ess / n1)) if np.isfinite(ess) and ess > 0 else 1.0
            res["re"] = self.evidence_finish(part, r, lstar, ess_factor, shape, lo, hi)["re"]
        res.update(shape=float(shape), n_data=int(n_data), n1=n1, n2=n2, d=d, ess_factor=1.0 if ess_factor is None else float(ess_factor),
                   transform=tuple(int(t) for t in tr), lstar=lstar, mean=mean, chol=chol)
        return res

    def evidence(self, samples, data, lo, hi, shape=None, transform=None, n_proposal=None, fit_fraction=0.5, seed=0, ess_factor=None):
        """The marginal likelihood of the device model (set_model) for the observation `data` from posterior draws `samples` — a
        kept trace (n, C, d) or a flat pool (n, d) / (n,), d = 1 (Dc) or 3 (Dc, a, b), sampled with n0 = 0 inside the box (lo, hi)
        — by bridge sampling: the first fit_fraction of the rows fit a Gaussian proposal (pool_joint, in the coordinates of
        `transform`), the rest enter the estimator with n_proposal (default: as many) proposal draws; one more forward solve
        per draw (evidence_logtarget).  → dict(log_integral, log_evidence, re, iterations, n2_in_box, converged, shape, n_data,
        n1, n2, d, ess_factor, transform, lstar, mean, chol).  ess_factor (effective over actual number of posterior draws): by
        default, for a kept trace, from diagnostics' ESS of the series f2; for a flat pool 1."""
        self._need_model()
        shape = 0.5 * self.nout if shape is None else float(shape)
        obs = self._in(data)
        return self._evidence(samples, lambda theta, logg: self.evidence_logtarget(theta, obs, lo, hi, logg, shape, transform), lo, hi,
                              shape, self.nout, transform, n_proposal, fit_fraction, seed, ess_factor)

    def evidence_from_ssq(self, samples, ssq_fn, lo, hi, shape, transform=None, n_proposal=None, fit_fraction=0.5, seed=0, ess_factor=None,
                          n_data=None):
        """evidence with the caller's sum of squares: ssq_fn(q (m, d) float64 on the host) → SSq (m,), called for points strictly
        inside the box only — any object under the project's model contract, or a closed form.  shape is the sampler's
        (n_data / 2 at n0 = 0; n_data defaults to 2 shape).  The proposal, its density and the bridge run on the GPU."""
        shape = float(shape)
        d = int(np.shape(samples)[-1]) if np.ndim(samples) > 1 else 1
        tr = self._ev_flags(transform, d)
        blo, bhi = _vec(lo, d, "lo"), _vec(hi, d, "hi")

        def ltarget(theta, logg):
            q, g = _host(theta).reshape(-1, d), _host(logg).reshape(-1)
            inb = np.all((q > blo) & (q < bhi), axis=1)
            l = np.full(q.shape[0], -np.inf)
            if inb.any():
                ssq = np.asarray(ssq_fn(q[inb]), dtype=np.float64).reshape(-1)
                ok = np.isfinite(ssq) & (ssq > 0)
                jac = np.log(q[inb][:, tr == 1]).sum(axis=1)
                l[inb] = np.where(ok, -shape * np.log(np.where(ok, ssq, 1.0)) + jac - g[inb], -np.inf)
            return l

        return self._evidence(samples, ltarget, lo, hi, shape, int(round(2 * shape)) if n_data is None else n_data, transform, n_proposal,
                              fit_fraction, seed, ess_factor)

    # -- tempered sequential Monte Carlo over the box prior (include/rsf_smc.h) ------------------------------
    def _smc_box(self, lo, hi, d=None):
        d = int(np.size(lo)) if d is None else int(d)
        return _vec(lo, d, "lo"), _vec(hi, d, "hi"), d

    def _smc_particles(self, q, l=None):
        """q (n,) or (n, d) and l (n,) in this engine's memory space → (q (n, d), l, n, d)"""
        q = self._in(q)
        if q.ndim == 1:
            q = q.reshape(-1, 1)
        n, d = int(q.shape[0]), int(q.shape[1])
        l = self._in(l)
        if l is not None and math.prod(l.shape) != n:
            raise ValueError(f"l holds {math.prod(l.shape)} values, q {n} particles")
        return q, l, n, d

    def _bytes(self, x):
        """a uint8 array in this engine's memory space"""
        if self.mem == "device":
            t = self._torch
            return (x if isinstance(x, t.Tensor) else t.as_tensor(np.ascontiguousarray(x, dtype=np.uint8))).to(device=f"cuda:{self.device}", dtype=t.uint8).contiguous()
        return np.ascontiguousarray(x, dtype=np.uint8)

    def smc_init(self, lo, hi, n, seed=0, offset=0):
        """rsf_smc_init: n particles uniform in the strict box (lo, hi) → q (n, d) in this engine's memory space.  Particle j uses
        the Philox stream of (seed, offset + j, iteration 0): shards with offsets form one stream."""
        lo, hi, d = self._smc_box(lo, hi)
        q = self._empty((max(int(n), 0), d))
        _abi.check(self.lib, self.lib.rsf_smc_init(self._ctx, int(n), d, _dp(lo), _dp(hi), int(seed), int(offset), self._ptr(q)))
        return q

    def smc_weight_sums(self, l, deltas, lmax=None):
        """rsf_smc_weight_sums: for up to SMC_MAX_CANDIDATES steps `deltas`, in one read of l (n,) → dict(lmax, n_finite, n_neginf,
        sums (m, 2): the sum of w = exp(delta (l - lmax)) and of w^2 per candidate).  lmax: by default the largest finite l;
        shards of one population pass the population's, and their sums then add."""
        x = self._in(l)
        dl = np.ascontiguousarray(np.atleast_1d(np.asarray(deltas, dtype=np.float64)))
        if dl.ndim != 1 or not 1 <= dl.size <= _abi.SMC_MAX_CANDIDATES:
            raise ValueError(f"deltas holds 1 to {_abi.SMC_MAX_CANDIDATES} steps")
        out = np.empty(_abi.SMC_HEAD + 2 * dl.size)
        _abi.check(self.lib, self.lib.rsf_smc_weight_sums(self._ctx, math.prod(x.shape), self._ptr(x), int(dl.size), _dp(dl),
                                                          float("nan") if lmax is None else float(lmax), _dp(out)))
        return {"lmax": float(out[0]), "n_finite": int(out[1]), "n_neginf": int(out[2]), "sums": out[_abi.SMC_HEAD:].reshape(-1, 2).copy()}

    def smc_next_delta(self, l, beta, ess_fraction=0.5):
        """The next temperature step from beta: the largest delta <= 1 - beta that keeps the effective sample size of the weights
        exp(delta (l - lmax)) at ess_fraction of the particles with a finite l, by SMC_ROUNDS rounds of 16-section, each one read of
        l (rsf_smc_weight_sums, rsf_smc_section) → dict(delta, beta (the next; exactly 1.0 at the end), lmax, sum_w, ess)."""
        x = self._in(l)
        search = _DeltaSearch(self.lib, beta, ess_fraction)
        while not search.update(self.smc_weight_sums(x, search.candidates())):
            pass
        return search.out

    def smc_stage_uniform(self, seed, stage):
        """The resampling uniform of a stage: u53 of the first two Philox words of the counter (2^32 - 1, 2^32 - 1, stage, 4)."""
        plo, phi, slot = _abi.SMC_RESAMPLE_COUNTER
        w = self.philox((plo, phi, int(stage), slot), (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF))
        return ((((w[0] << 32) | w[1]) >> 11) + 1) * 2.0 ** -53

    def smc_resample(self, q, l, delta, lmax, u):
        """rsf_smc_resample: systematic resampling with the weights exp(delta (l - lmax)) and the uniform u in (0, 1] →
        (cum (n,), ancestors (n,) int64, q (n, d) and l (n,) gathered through the ancestors) in this engine's memory space."""
        q, l, n, d = self._smc_particles(q, l)
        if l is None:
            raise ValueError("l is (n,)")
        cum, qo, lo_ = self._empty((n,)), self._empty((n, d)), self._empty((n,))
        anc = self._torch.empty((n,), dtype=self._torch.int64, device=f"cuda:{self.device}") if self.mem == "device" else np.empty(n, dtype=np.int64)
        _abi.check(self.lib, self.lib.rsf_smc_resample(self._ctx, n, d, self._ptr(q), self._ptr(l), float(delta), float(lmax), float(u),
                                                       self._ptr(cum), self._ptr(anc), self._ptr(qo), self._ptr(lo_)))
        return cum, anc, qo, lo_

    def _smc_chol(self, chol, d):
        L = _host(chol).reshape(-1)
        if L.size != d * d:
            raise ValueError(f"chol is ({d}, {d})")
        return L

    def smc_move(self, q, l, data, lo, hi, chol, beta, seed=0, offset=0, iter0=1, steps=3, shape=None):
        """rsf_smc_move, the fused hot path: `steps` Metropolis steps per particle on pi_beta with the proposal N(q, chol chol^T),
        each one float64 RK4 solve of the device model against `data` → (q (n, d), l (n,), accepted (steps,) int64); the arrays
        handed in are not changed.  Step k uses the variates of draws(seed, offset + j, iter0 + k, d)."""
        self._need_model()
        q, l, n, d = self._smc_particles(q, l)
        obs = self._in(data)
        if obs.ndim != 1 or int(obs.shape[0]) != self.nout:
            raise ValueError(f"data has shape {tuple(obs.shape)}, the model produces {self.nout} samples")
        lo, hi, _ = self._smc_box(lo, hi, d)
        L = self._smc_chol(chol, d)
        q, l = (q.clone(), l.clone()) if hasattr(q, "clone") else (q.copy(), l.copy())
        acc = np.zeros(max(int(steps), 1), dtype=np.int64)
        _abi.check(self.lib, self.lib.rsf_smc_move(self._ctx, n, d, self._ptr(q), self._ptr(l), self._ptr(obs),
                                                   float(0.5 * self.nout if shape is None else shape), _dp(lo), _dp(hi), _dp(L), float(beta),
                                                   int(seed), int(offset), int(iter0), int(steps), acc.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        return q, l, acc

    def smc_move_propose(self, q, lo, hi, chol, seed=0, offset=0, iteration=1):
        """rsf_smc_move_propose: the proposals of one Metropolis step → (q_new (n, d), inbox (n,) uint8)."""
        q, _, n, d = self._smc_particles(q)
        lo, hi, _ = self._smc_box(lo, hi, d)
        L = self._smc_chol(chol, d)
        qn, inb = self._empty((n, d)), self._empty((n,), np.uint8)
        _abi.check(self.lib, self.lib.rsf_smc_move_propose(self._ctx, n, d, self._ptr(q), _dp(lo), _dp(hi), _dp(L), int(seed), int(offset),
                                                           int(iteration), self._ptr(qn), self._ptr(inb)))
        return qn, inb

    def smc_move_accept(self, q, l, q_new, inbox, ssq_new, shape, beta, seed=0, offset=0, iteration=1):
        """rsf_smc_move_accept: the accept test of one Metropolis step with the caller's sums of squares ssq_new (n,), read where
        inbox is 1 → (q (n, d), l (n,), accepted); the arrays handed in are not changed."""
        q, l, n, d = self._smc_particles(q, l)
        qn, ssq, inb = self._in(q_new), self._in(ssq_new), self._bytes(inbox)
        if math.prod(qn.shape) != n * d or math.prod(ssq.shape) != n or math.prod(inb.shape) != n:
            raise ValueError(f"q_new is ({n}, {d}), inbox and ssq_new ({n},)")
        q, l = (q.clone(), l.clone()) if hasattr(q, "clone") else (q.copy(), l.copy())
        acc = ctypes.c_int64()
        _abi.check(self.lib, self.lib.rsf_smc_move_accept(self._ctx, n, d, self._ptr(q), self._ptr(l), self._ptr(qn), self._ptr(inb), self._ptr(ssq),
                                                          float(shape), float(beta), int(seed), int(offset), int(iteration), ctypes.byref(acc)))
        return q, l, int(acc.value)

    def smc_std2(self, l, shape, seed=0, offset=0, iteration=0):
        """rsf_smc_std2: sigma^2 of the final particles from InvGamma(shape, SSq / 2), SSq = exp(-l / shape) → (n,)."""
        x = self._in(l)
        out = self._empty((math.prod(x.shape),))
        _abi.check(self.lib, self.lib.rsf_smc_std2(self._ctx, math.prod(x.shape), self._ptr(x), float(shape), int(seed), int(offset), int(iteration),
                                                   self._ptr(out)))
        return out

    def _smc(self, lo, hi, n, shape, seed, offset, ess_fraction, steps, max_stages, ltarget, move, history):
        """What smc and smc_from_ssq share.  ltarget(q (n, d)) → l (n,); move(q, l, chol, beta, iter0) → (q, l, accepted, solves)."""
        lo, hi, d = self._smc_box(lo, hi)
        n, steps, shape = int(n), int(steps), float(shape)
        if d not in (1, 3):
            raise ValueError("the box has d = 1 (Dc) or 3 (Dc, a, b) parameters")
        if not 0.0 < float(ess_fraction) < 1.0 or not 1 <= steps <= _abi.SMC_MAX_STEPS or int(max_stages) < 1:
            raise ValueError(f"ess_fraction lies strictly inside (0, 1), steps in [1, {_abi.SMC_MAX_STEPS}], max_stages >= 1")
        q = self.smc_init(lo, hi, n, seed, offset)
        l = ltarget(q)
        logi, beta, stages, hist, solves = float(np.log(hi - lo).sum()), 0.0, [], [], n
        inc = ctypes.c_double()
        while beta < 1.0:
            s = len(stages)
            if s >= int(max_stages):
                raise _abi.RsfError(-1, f"Engine.smc: beta = {beta!r} after max_stages = {max_stages} stages")
            nd = self.smc_next_delta(l, beta, ess_fraction)
            _abi.check(self.lib, self.lib.rsf_smc_increment(n, nd["sum_w"], nd["delta"], nd["lmax"], ctypes.byref(inc)))
            logi, beta = logi + inc.value, nd["beta"]
            u = self.smc_stage_uniform(seed, s)
            cum, anc, q, l = self.smc_resample(q, l, nd["delta"], nd["lmax"], u)
            cov = self.pool_joint(q)["cov"] if n > 1 else np.zeros((d, d))
            if not np.isfinite(cov).all():
                raise _abi.RsfError(-1, "Engine.smc: the resampled particles' covariance is not finite")
            chol = np.linalg.cholesky((2.38 ** 2 / d) * cov + np.diag((1e-6 * (hi - lo)) ** 2))
            q, l, acc, ns, after = move(q, l, chol, beta, s * steps + 1)
            solves += ns
            stages.append({"beta": beta, "delta": nd["delta"], "ess": nd["ess"], "accept_rate": float(np.sum(acc)) / (n * steps),
                           "log_integral": logi})
            if history:
                hist.append({"lmax": nd["lmax"], "u": u, "cum": _host(cum), "ancestors": np.asarray(anc.cpu() if hasattr(anc, "cpu") else anc),
                             "chol": chol, "after": after})
        std2 = self.smc_std2(l, shape, seed, offset, len(stages) * steps + 1)
        ev = ctypes.c_double()
        _abi.check(self.lib, self.lib.rsf_smc_log_evidence(logi, shape, d, _dp(lo), _dp(hi), ctypes.byref(ev)))
        out = {"q": q, "l": l, "std2": std2, "log_integral": logi, "log_evidence": ev.value, "stages": stages, "n_solves": solves,
               "shape": shape, "d": d, "n": n}
        if history:
            out["history"] = hist
        return out

    def smc(self, data, lo, hi, n, shape=None, seed=0, offset=0, ess_fraction=0.5, steps=3, max_stages=200, history=False):
        """Tempered sequential Monte Carlo for the device model (set_model) and the observation `data` over the strict box (lo, hi),
        d = 1 (Dc) or 3 (Dc, a, b): n particles start uniform in the box — no start point, no burn-in — and move through
        SSq^(-shape beta), beta from 0 to 1; each stage chooses its temperature step from the weights' effective sample size
        (ess_fraction), resamples systematically and takes `steps` Metropolis steps per particle with the population's own
        covariance (pool_joint), one forward solve each (smc_move).  → dict(q (n, d), l (n,) = -shape log SSq, std2 (n,) — an
        equally weighted sample of the sampler's target —, log_integral, log_evidence (the constants of evidence_finish), stages
        [dict(beta, delta, ess, accept_rate, log_integral so far)], n_solves, shape, d, n).  shape defaults to nout / 2."""
        self._need_model()
        shape = 0.5 * self.nout if shape is None else float(shape)
        obs = self._in(data)
        blo, bhi, d = self._smc_box(lo, hi)

        def move(q, l, chol, beta, iter0):
            q, l, acc = self.smc_move(q, l, obs, blo, bhi, chol, beta, seed, offset, iter0, steps, shape)
            return q, l, acc, int(n) * int(steps), [(_host(q), _host(l))] if history else None

        return self._smc(lo, hi, n, shape, seed, offset, ess_fraction, steps, max_stages,
                         lambda q: self.evidence_logtarget(q, obs, blo, bhi, self._in(np.zeros(int(n))), shape), move, history)

    def smc_from_ssq(self, ssq_fn, lo, hi, n, shape, seed=0, offset=0, ess_fraction=0.5, steps=3, max_stages=200, history=False):
        """smc with the caller's sum of squares: ssq_fn(q (m, d) float64 on the host) → SSq (m,), called for points strictly inside
        the box only.  The start, the weights, the resampling, the proposals and the accept tests run on the GPU."""
        shape = float(shape)
        blo, bhi, d = self._smc_box(lo, hi)

        def ltarget(q):
            ssq = np.asarray(ssq_fn(_host(q).reshape(-1, d)), dtype=np.float64).reshape(-1)
            ok = np.isfinite(ssq) & (ssq > 0)
            return self._in(np.where(ok, -shape * np.log(np.where(ok, ssq, 1.0)), -np.inf))

        def move(q, l, chol, beta, iter0):
            accs, solves, after = [], 0, []
            for k in range(int(steps)):
                qn, inb = self.smc_move_propose(q, blo, bhi, chol, seed, offset, iter0 + k)
                hq, hi_ = _host(qn).reshape(-1, d), np.asarray(inb.cpu() if hasattr(inb, "cpu") else inb).astype(bool)
                ssq = np.zeros(hq.shape[0])
                if hi_.any():
                    ssq[hi_] = np.asarray(ssq_fn(hq[hi_]), dtype=np.float64).reshape(-1)
                q, l, a = self.smc_move_accept(q, l, qn, inb, ssq, shape, beta, seed, offset, iter0 + k)
                accs.append(a)
                solves += int(hi_.sum())
                if history:
                    after.append((_host(q), _host(l)))
            return q, l, accs, solves, after

        return self._smc(lo, hi, n, shape, seed, offset, ess_fraction, steps, max_stages, ltarget, move, history)

    # -- P independent SMC populations per call (include/rsf_smc_batch.h) --------------------------------------
    def _smc_batch_particles(self, q, l=None):
        """q (P, n) or (P, n, d) and l (P, n) in this engine's memory space → (q (P, n, d), l, P, n, d)"""
        q = self._in(q)
        if q.ndim == 2:
            q = q.reshape(int(q.shape[0]), int(q.shape[1]), 1)
        if q.ndim != 3:
            raise ValueError("the particles of P populations are (P, n, d)")
        P, n, d = (int(v) for v in q.shape)
        l = self._in(l)
        if l is not None and tuple(l.shape) != (P, n):
            raise ValueError(f"l has shape {tuple(l.shape)}, q {P} populations of {n} particles")
        return q, l, P, n, d

    def _smc_batch_data(self, data):
        """data (nout,) or (G, nout) in this engine's memory space → ((G, nout), G)"""
        obs = self._in(data)
        if obs.ndim == 1:
            obs = obs.reshape(1, -1)
        if obs.ndim != 2 or int(obs.shape[0]) < 1 or int(obs.shape[1]) != self.nout:
            raise ValueError(f"data has shape {tuple(obs.shape)}: (nout,) or (G, nout) with the model's nout = {self.nout}")
        return obs, int(obs.shape[0])

    @staticmethod
    def _smc_active(active, P):
        return np.ones(P, dtype=np.uint8) if active is None else _pop_array(np.asarray(active, dtype=bool), P, np.uint8, "active")

    def smc_batch_init(self, lo, hi, n, seeds, offsets=0):
        """rsf_smc_batch_init: smc_init for P = len(seeds) populations in one launch → q (P, n, d)."""
        lo, hi, d = self._smc_box(lo, hi)
        sd = np.ascontiguousarray(np.atleast_1d(np.asarray(seeds)).astype(np.uint64))
        P = int(sd.size)
        off = _pop_array(offsets, P, np.int64, "offsets")
        q = self._empty((P, max(int(n), 0), d))
        _abi.check(self.lib, self.lib.rsf_smc_batch_init(self._ctx, P, int(n), d, _dp(lo), _dp(hi), _ptr_of(sd, ctypes.c_uint64),
                                                         _ptr_of(off, ctypes.c_int64), self._ptr(q)))
        return q

    def smc_batch_logtarget(self, q, data, group, lo, hi, shape=None):
        """rsf_smc_batch_logtarget: l = -shape log SSq of every particle of q (P, n, d) against the row group[p] of data (G, nout),
        one solve each in one launch → (P, n); -inf outside the strict box."""
        self._need_model()
        q, _, P, n, d = self._smc_batch_particles(q)
        obs, G = self._smc_batch_data(data)
        lo, hi, _ = self._smc_box(lo, hi, d)
        grp = _pop_array(group, P, np.int32, "group")
        l = self._empty((P, n))
        _abi.check(self.lib, self.lib.rsf_smc_batch_logtarget(self._ctx, P, n, d, self._ptr(q), self._ptr(obs), G, _i32p(grp),
                                                              float(0.5 * self.nout if shape is None else shape), _dp(lo), _dp(hi), self._ptr(l)))
        return l

    def smc_batch_weight_sums(self, l, deltas, lmax=None, active=None):
        """rsf_smc_batch_weight_sums: smc_weight_sums of every active population of l (P, n) with its own steps deltas (P, m) (or
        (m,) for all) and lmax (P,) (None or NaN: the population's largest finite l) in one read → a list of smc_weight_sums'
        dicts, None for an inactive population."""
        x = self._in(l)
        if x.ndim != 2:
            raise ValueError("l is (P, n)")
        P, n = int(x.shape[0]), int(x.shape[1])
        dl = np.asarray(deltas, dtype=np.float64)
        dl = np.ascontiguousarray(np.broadcast_to(dl, (P, dl.shape[-1])) if dl.ndim == 1 else dl)
        if dl.ndim != 2 or dl.shape[0] != P or not 1 <= dl.shape[1] <= _abi.SMC_MAX_CANDIDATES:
            raise ValueError(f"deltas holds 1 to {_abi.SMC_MAX_CANDIDATES} steps for each of the {P} populations")
        m = int(dl.shape[1])
        lm = _pop_array(float("nan") if lmax is None else lmax, P, np.float64, "lmax")
        act = self._smc_active(active, P)
        out = np.zeros((P, _abi.SMC_HEAD + 2 * m))
        _abi.check(self.lib, self.lib.rsf_smc_batch_weight_sums(self._ctx, P, n, self._ptr(x), m, _dp(dl), _dp(lm), _ptr_of(act, ctypes.c_uint8), _dp(out)))
        return [{"lmax": float(o[0]), "n_finite": int(o[1]), "n_neginf": int(o[2]), "sums": o[_abi.SMC_HEAD:].reshape(-1, 2).copy()} if a else None
                for o, a in zip(out, act)]

    def smc_batch_next_delta(self, l, beta, ess_fraction=0.5, active=None):
        """smc_next_delta for every active population of l (P, n) from its own temperature beta (P,): each round of the search is
        one smc_batch_weight_sums over the populations still searching → a list of smc_next_delta's dicts, None for an inactive one."""
        x = self._in(l)
        P = int(x.shape[0])
        bt, act = _pop_array(beta, P, np.float64, "beta"), self._smc_active(active, P)
        search = [_DeltaSearch(self.lib, bt[p], ess_fraction) if act[p] else None for p in range(P)]
        todo = act.astype(bool)
        cand = np.zeros((P, _abi.SMC_MAX_CANDIDATES))
        while todo.any():
            for p in np.flatnonzero(todo):
                cand[p] = search[p].candidates()
            res = self.smc_batch_weight_sums(x, cand, None, todo)
            for p in np.flatnonzero(todo):
                todo[p] = not search[p].update(res[p])
        return [sr.out if sr is not None else None for sr in search]

    def smc_batch_resample(self, q, l, delta, lmax, u, active=None, out=None):
        """rsf_smc_batch_resample: smc_resample of every active population of q (P, n, d), l (P, n) with its delta, lmax and u (P,)
        → (cum (P, n), ancestors (P, n) int64, local to the population, q (P, n, d) and l (P, n) gathered).  An inactive
        population's q and l are copied through and its rows of cum and ancestors are left as they are (zero in fresh buffers;
        out = (cum, ancestors, q_out, l_out) supplies the buffers)."""
        q, l, P, n, d = self._smc_batch_particles(q, l)
        if l is None:
            raise ValueError("l is (P, n)")
        dl, lm, uu = (_pop_array(v, P, np.float64, w) for v, w in ((delta, "delta"), (lmax, "lmax"), (u, "u")))
        act = self._smc_active(active, P)
        if out is None:
            cum, qo, lo_ = self._empty((P, n)), self._empty((P, n, d)), self._empty((P, n))
            anc = self._torch.empty((P, n), dtype=self._torch.int64, device=f"cuda:{self.device}") if self.mem == "device" else np.empty((P, n), dtype=np.int64)
            for x in (cum, anc):
                x.fill_(0) if hasattr(x, "fill_") else x.fill(0)
        else:
            cum, anc, qo, lo_ = out
        _abi.check(self.lib, self.lib.rsf_smc_batch_resample(self._ctx, P, n, d, self._ptr(q), self._ptr(l), _dp(dl), _dp(lm), _dp(uu),
                                                             _ptr_of(act, ctypes.c_uint8), self._ptr(cum), self._ptr(anc), self._ptr(qo), self._ptr(lo_)))
        return cum, anc, qo, lo_

    def smc_batch_move(self, q, l, data, group, lo, hi, chol, beta, seeds, offsets=0, iter0=1, steps=3, shape=None, active=None, inplace=False):
        """rsf_smc_batch_move, the fused hot path for P populations in ONE launch: population p takes `steps` Metropolis steps on
        pi_beta[p] against the row group[p] of data (G, nout) with the proposal factor chol[p] (P, d, d), the stream (seeds[p],
        offsets[p]) and the first iteration iter0[p] → (q (P, n, d), l (P, n), accepted (P, steps) int64).  The arrays handed in are
        not changed unless inplace; an inactive population is not touched (its accepted counts read 0)."""
        self._need_model()
        q, l, P, n, d = self._smc_batch_particles(q, l)
        if l is None:
            raise ValueError("l is (P, n)")
        obs, G = self._smc_batch_data(data)
        lo, hi, _ = self._smc_box(lo, hi, d)
        L = _host(chol).reshape(-1)
        if L.size != P * d * d:
            raise ValueError(f"chol is ({P}, {d}, {d})")
        grp, bt = _pop_array(group, P, np.int32, "group"), _pop_array(beta, P, np.float64, "beta")
        sd, off, it = _pop_array(seeds, P, np.uint64, "seeds"), _pop_array(offsets, P, np.int64, "offsets"), _pop_array(iter0, P, np.int64, "iter0")
        act = self._smc_active(active, P)
        if not inplace:
            q, l = (q.clone(), l.clone()) if hasattr(q, "clone") else (q.copy(), l.copy())
        acc = np.zeros((P, max(int(steps), 1)), dtype=np.int64)
        _abi.check(self.lib, self.lib.rsf_smc_batch_move(self._ctx, P, n, d, self._ptr(q), self._ptr(l), self._ptr(obs), G, _i32p(grp),
                                                         float(0.5 * self.nout if shape is None else shape), _dp(lo), _dp(hi), _dp(L), _dp(bt),
                                                         _ptr_of(sd, ctypes.c_uint64), _ptr_of(off, ctypes.c_int64), _ptr_of(it, ctypes.c_int64),
                                                         int(steps), _ptr_of(act, ctypes.c_uint8), _ptr_of(acc, ctypes.c_int64)))
        return q, l, acc

    def smc_batch_std2(self, l, shape, seeds, offsets=0, iteration=0):
        """rsf_smc_batch_std2: smc_std2 of every population of l (P, n) with its own stream and iteration → (P, n)."""
        x = self._in(l)
        if x.ndim != 2:
            raise ValueError("l is (P, n)")
        P, n = int(x.shape[0]), int(x.shape[1])
        sd, off, it = _pop_array(seeds, P, np.uint64, "seeds"), _pop_array(offsets, P, np.int64, "offsets"), _pop_array(iteration, P, np.int64, "iteration")
        out = self._empty((P, n))
        _abi.check(self.lib, self.lib.rsf_smc_batch_std2(self._ctx, P, n, self._ptr(x), float(shape), _ptr_of(sd, ctypes.c_uint64),
                                                         _ptr_of(off, ctypes.c_int64), _ptr_of(it, ctypes.c_int64), self._ptr(out)))
        return out

    def smc_batch(self, data, lo, hi, n, groups=None, seeds=None, offsets=None, replicates=1, shape=None, ess_fraction=0.5, steps=3,
                  max_stages=200, history=False):
        """Engine.smc for many independent populations at once: every row of `groups` of data (nout,) or (G, nout) x `replicates`
        (smc_batch_populations: by default replicate r has seed r and offset 0), each with its own temperature ladder, stage
        count, resampling uniforms and proposal covariance, every stage ONE launch per kernel over the populations still below
        beta = 1 (a population that reaches it goes inactive).  Each population's result equals, bit for bit, Engine.smc with
        its seed, offset and data row.  → dict(runs: a list of Engine.smc's dicts — plus group, replicate, seed, offset —, the
        replicates of a group next to each other; summary: smc_batch_summary of their log evidences, per group)."""
        self._need_model()
        obs, G = self._smc_batch_data(data)
        pops = smc_batch_populations(G, groups, seeds, offsets, replicates)
        grp, sd, off = pops["group"], pops["seed"], pops["offset"]
        P = int(grp.size)
        lo, hi, d = self._smc_box(lo, hi)
        n, steps, shape = int(n), int(steps), 0.5 * self.nout if shape is None else float(shape)
        if d not in (1, 3):
            raise ValueError("the box has d = 1 (Dc) or 3 (Dc, a, b) parameters")
        if not 0.0 < float(ess_fraction) < 1.0 or not 1 <= steps <= _abi.SMC_MAX_STEPS or int(max_stages) < 1:
            raise ValueError(f"ess_fraction lies strictly inside (0, 1), steps in [1, {_abi.SMC_MAX_STEPS}], max_stages >= 1")
        q = self.smc_batch_init(lo, hi, n, sd, off)
        l = self.smc_batch_logtarget(q, obs, grp, lo, hi, shape)
        logi, beta = np.full(P, float(np.log(hi - lo).sum())), np.zeros(P)
        stages, hist = [[] for _ in range(P)], [[] for _ in range(P)]
        delta, lmax, u, chol = np.zeros(P), np.zeros(P), np.ones(P), np.tile(np.eye(d), (P, 1, 1))
        inc = ctypes.c_double()
        active = beta < 1.0
        while active.any():
            live = np.flatnonzero(active)
            for p in live:
                if len(stages[p]) >= int(max_stages):
                    raise _abi.RsfError(-1, f"Engine.smc_batch: population {p}: beta = {beta[p]!r} after max_stages = {max_stages} stages")
            nd = self.smc_batch_next_delta(l, beta, ess_fraction, active)
            for p in live:
                _abi.check(self.lib, self.lib.rsf_smc_increment(n, nd[p]["sum_w"], nd[p]["delta"], nd[p]["lmax"], ctypes.byref(inc)))
                logi[p], beta[p], delta[p], lmax[p] = logi[p] + inc.value, nd[p]["beta"], nd[p]["delta"], nd[p]["lmax"]
                u[p] = self.smc_stage_uniform(int(sd[p]), len(stages[p]))
            cum, anc, q, l = self.smc_batch_resample(q, l, delta, lmax, u, active)
            for p in live:
                cov = self.pool_joint(q[p])["cov"] if n > 1 else np.zeros((d, d))
                if not np.isfinite(cov).all():
                    raise _abi.RsfError(-1, f"Engine.smc_batch: population {p}: the resampled particles' covariance is not finite")
                chol[p] = np.linalg.cholesky((2.38 ** 2 / d) * cov + np.diag((1e-6 * (hi - lo)) ** 2))
            it0 = np.array([len(st) * steps + 1 for st in stages], dtype=np.int64)
            q, l, acc = self.smc_batch_move(q, l, obs, grp, lo, hi, chol, np.where(active, beta, 1.0), sd, off, it0, steps, shape, active, inplace=True)
            for p in live:
                stages[p].append({"beta": float(beta[p]), "delta": float(delta[p]), "ess": nd[p]["ess"],
                                  "accept_rate": float(np.sum(acc[p])) / (n * steps), "log_integral": float(logi[p])})
                if history:
                    hist[p].append({"lmax": float(lmax[p]), "u": float(u[p]), "cum": _host(cum[p]),
                                    "ancestors": np.asarray(anc[p].cpu() if hasattr(anc, "cpu") else anc[p]).copy(), "chol": chol[p].copy(),
                                    "after": [(_host(q[p]).copy(), _host(l[p]).copy())]})
            active = beta < 1.0
        std2 = self.smc_batch_std2(l, shape, sd, off, [len(st) * steps + 1 for st in stages])
        ev, runs = ctypes.c_double(), []
        for p in range(P):
            _abi.check(self.lib, self.lib.rsf_smc_log_evidence(float(logi[p]), shape, d, _dp(lo), _dp(hi), ctypes.byref(ev)))
            runs.append({"q": q[p], "l": l[p], "std2": std2[p], "log_integral": float(logi[p]), "log_evidence": ev.value, "stages": stages[p],
                         "n_solves": n * (1 + steps * len(stages[p])), "shape": shape, "d": d, "n": n, "group": int(grp[p]),
                         "replicate": int(pops["replicate"][p]), "seed": int(sd[p]), "offset": int(off[p])})
            if history:
                runs[-1]["history"] = hist[p]
        return {"runs": runs, "summary": smc_batch_summary([r["log_evidence"] for r in runs], grp)}

    # -- multi-start Levenberg-Marquardt least squares (include/rsf_fit.h) ----------------------------------------
    def _ints(self, x):
        """an int32 array in this engine's memory space"""
        if self.mem == "device":
            t = self._torch
            return t.as_tensor(np.ascontiguousarray(x, dtype=np.int32)).to(device=f"cuda:{self.device}")
        return np.array(x, dtype=np.int32)

    @staticmethod
    def _fit_args(q0, lo, hi, dims, fd_rel_step, ftol, max_iter, iters_per_launch):
        """The checks Engine.fit and fit_from_residuals share → (q0 (n, d) a fresh host array, lo, hi, d, fd, ftol, max_iter, iters_per_launch)"""
        q0 = _host(q0).copy()
        if q0.ndim == 1:
            q0 = q0.reshape(-1, 1)
        if q0.ndim != 2 or q0.shape[0] < 1 or q0.shape[1] not in dims:
            raise ValueError(f"q0 has shape {q0.shape}: (n,) or (n, d) start points, d one of {dims}")
        d = int(q0.shape[1])
        lo, hi = _vec(lo, d, "lo"), _vec(hi, d, "hi")
        if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (lo < hi).all()):
            raise ValueError("the box needs finite lo < hi in every parameter")
        fd = (1e-6 if d == 1 else 1e-4) if fd_rel_step is None else float(fd_rel_step)
        ftol, max_iter, ipl = float(ftol), int(max_iter), int(iters_per_launch)
        if not (math.isfinite(fd) and fd > 0.0 and math.isfinite(ftol) and ftol >= 0.0 and max_iter >= 1 and 1 <= ipl <= _abi.FIT_MAX_ITER):
            raise ValueError(f"fd_rel_step is finite and > 0, ftol finite and >= 0, max_iter >= 1, iters_per_launch in [1, {_abi.FIT_MAX_ITER}]")
        return q0, lo, hi, d, fd, ftol, max_iter, ipl

    def fit_normal(self, q, data, fd_rel_step=None):
        """rsf_fit_normal: the normal equations of the device model at the points q (n,) or (n, d), d = 1 (Dc) or 3 (Dc, a, b),
        against data (nout,) or (G, nout) (the points split evenly over the G series in order; G > 1: n / G a whole multiple of a
        workgroup's threads) → (ssq (n,), grad (n, d), jtj (n, d, d)) in this engine's memory space."""
        self._need_model()
        q = self._in(q)
        if q.ndim == 1:
            q = q.reshape(-1, 1)
        n, d = int(q.shape[0]), int(q.shape[1])
        obs = self._in(data)
        if obs.ndim not in (1, 2) or int(obs.shape[-1]) != self.nout:
            raise ValueError(f"data has shape {tuple(obs.shape)}: (nout,) or (G, nout), the model produces nout = {self.nout} samples")
        G = int(obs.shape[0]) if obs.ndim == 2 else 1
        fd = (1e-6 if d == 1 else 1e-4) if fd_rel_step is None else float(fd_rel_step)
        ssq, grad, jtj = self._empty((n,)), self._empty((n, d)), self._empty((n, d, d))
        _abi.check(self.lib, self.lib.rsf_fit_normal(self._ctx, n, d, self._ptr(q), self._ptr(obs), G, fd, self._ptr(ssq), self._ptr(grad), self._ptr(jtj)))
        return ssq, grad, jtj

    def _fit_state(self, q, grad, jtj, lam, status, ssq=None, iters=None):
        """The check of a fit state handed to the low-level calls, which read and write it through raw addresses: q (n, d), grad
        (n, d), jtj (n, d, d), lam (n,) and ssq (n,) float64, status (n,) and iters (n,) int32, each a C-contiguous array of this
        engine's memory space (a NumPy array, or a torch tensor on its device) → (n, d)"""
        if getattr(q, "ndim", 0) != 2:
            raise ValueError("q is (n, d)")
        n, d = int(q.shape[0]), int(q.shape[1])
        t = self._torch
        for what, x, shape, dt in (("q", q, (n, d), "float64"), ("grad", grad, (n, d), "float64"), ("jtj", jtj, (n, d, d), "float64"),
                                   ("lam", lam, (n,), "float64"), ("ssq", ssq, (n,), "float64"), ("status", status, (n,), "int32"),
                                   ("iters", iters, (n,), "int32")):
            if x is None and what in ("ssq", "iters"):
                continue
            if self.mem == "device":
                good = isinstance(x, t.Tensor) and x.is_cuda and x.is_contiguous() and str(x.dtype) == "torch." + dt
            else:
                good = isinstance(x, np.ndarray) and x.flags["C_CONTIGUOUS"] and x.dtype == np.dtype(dt)
            if not good or tuple(x.shape) != shape:
                raise ValueError(f"{what} must be a C-contiguous {dt} array of shape {shape} in this engine's memory space ({self.mem})")
        return n, d

    def fit_run(self, q, data, lo, hi, ssq, grad, jtj, lam, status, iters, n_iter, fd_rel_step=None, ftol=1e-9):
        """rsf_fit_run, the fused hot path: n_iter iterations of every RUNNING start IN PLACE in q (n, d), ssq, grad, jtj, lam,
        status and iters (int32), contiguous arrays of this engine's memory space as fit_normal leaves them."""
        self._need_model()
        n, d = self._fit_state(q, grad, jtj, lam, status, ssq, iters)
        data = self._in(data)
        G = int(data.shape[0]) if data.ndim == 2 else 1
        fd = (1e-6 if d == 1 else 1e-4) if fd_rel_step is None else float(fd_rel_step)
        _abi.check(self.lib, self.lib.rsf_fit_run(self._ctx, n, d, self._ptr(q), self._ptr(data), G, _dp(_vec(lo, d, "lo")), _dp(_vec(hi, d, "hi")), fd,
                                                  float(ftol), int(n_iter), self._ptr(ssq), self._ptr(grad), self._ptr(jtj), self._ptr(lam),
                                                  self._ptr(status), self._ptr(iters)))

    def fit_trial(self, q, grad, jtj, lam, status, lo, hi):
        """rsf_fit_trial: the trial points of the RUNNING starts → (q_trial (n, d), ok (n,) uint8)."""
        n, d = self._fit_state(q, grad, jtj, lam, status)
        qt, ok = self._empty((n, d)), self._empty((n,), np.uint8)
        _abi.check(self.lib, self.lib.rsf_fit_trial(self._ctx, n, d, self._ptr(q), self._ptr(grad), self._ptr(jtj), self._ptr(lam), _dp(_vec(lo, d, "lo")),
                                                    _dp(_vec(hi, d, "hi")), self._ptr(status), self._ptr(qt), self._ptr(ok)))
        return qt, ok

    def fit_decide(self, q, ssq, grad, jtj, lam, status, iters, q_trial, ok, ssq_new, grad_new, jtj_new, ftol=1e-9):
        """rsf_fit_decide: accept or reject the trial points with the caller's normal equations there, IN PLACE in q, ssq, grad,
        jtj, lam, status and iters (contiguous arrays of this engine's memory space); q_trial (n, d), ok (n,), ssq_new (n,), grad_new
        (n, d) and jtj_new (n, d, d) are read and may have any layout."""
        n, d = self._fit_state(q, grad, jtj, lam, status, ssq, iters)
        q_trial, ok, ssq_new, grad_new, jtj_new = self._in(q_trial), self._bytes(ok), self._in(ssq_new), self._in(grad_new), self._in(jtj_new)
        if (tuple(q_trial.shape), tuple(ok.shape), tuple(ssq_new.shape), tuple(grad_new.shape), tuple(jtj_new.shape)) != ((n, d), (n,), (n,), (n, d), (n, d, d)):
            raise ValueError(f"q_trial and grad_new are ({n}, {d}), ok and ssq_new ({n},), jtj_new ({n}, {d}, {d})")
        _abi.check(self.lib, self.lib.rsf_fit_decide(self._ctx, n, d, self._ptr(q), self._ptr(ssq), self._ptr(grad), self._ptr(jtj), self._ptr(lam),
                                                     self._ptr(status), self._ptr(iters), self._ptr(q_trial), self._ptr(ok), self._ptr(ssq_new),
                                                     self._ptr(grad_new), self._ptr(jtj_new), float(ftol)))

    @staticmethod
    def _ints_host(x):
        return np.asarray(x.cpu() if hasattr(x, "cpu") else x)

    def _fit_result(self, keep, q, ssq, grad, jtj, lam, status, iters, n_groups, n_obs):
        return FitResult(self.lib, _host(q)[keep], _host(ssq)[keep], _host(grad)[keep], _host(jtj)[keep], _host(lam)[keep],
                         self._ints_host(status)[keep].astype(np.int32), self._ints_host(iters)[keep].astype(np.int32), n_groups, n_obs)

    def fit(self, q0, data, lo, hi, fd_rel_step=None, ftol=1e-9, max_iter=100, iters_per_launch=8):
        """Multi-start Levenberg-Marquardt least squares of the device model (set_model) against `data` over the strict box
        (lo, hi): q0 (n,) or (n, d) start points, d = 1 (Dc) or 3 (Dc, a, b); data (nout,), or (G, nout) with the starts split
        evenly over the G series in order.  Every start iterates on the GPU (rsf_fit_run, iters_per_launch iterations per launch,
        one group solve each) until it is CONVERGED (a relative decrease of ssq below ftol), STALLED or max_iter is reached; only
        the statuses are read between launches.  fd_rel_step: the forward-difference step of the sensitivities, by default 1e-6
        at d = 1 and 1e-4 at d = 3 (sample_batched's).  → FitResult.  With G > 1 each series' starts are padded to whole
        workgroups with copies of its first start; the result holds the caller's starts only."""
        self._need_model()
        return self._fit_drive(self.fit_normal, self.fit_run, q0, data, lo, hi, fd_rel_step, ftol, max_iter, iters_per_launch)

    def _fit_drive(self, normal, run, q0, data, lo, hi, fd_rel_step, ftol, max_iter, iters_per_launch, ready=None):
        """Engine.fit's driver, shared with law_fit: normal(q, obs, fd) and run(q, obs, lo, hi, ssq, grad, jtj, lam, status, iters, k,
        fd, ftol) are fit_normal's and fit_run's signatures; ready() is called after the argument checks and before the first launch"""
        q0, lo, hi, d, fd, ftol, max_iter, ipl = self._fit_args(q0, lo, hi, (1, 3), fd_rel_step, ftol, max_iter, iters_per_launch)
        obs = _host(data)
        obs = obs.reshape(1, -1) if obs.ndim == 1 else obs
        if obs.ndim != 2 or obs.shape[1] != self.nout:
            raise ValueError(f"data has shape {obs.shape}: (nout,) or (G, nout), the model produces nout = {self.nout} samples")
        n, G = q0.shape[0], obs.shape[0]
        if n % G:
            raise ValueError(f"{n} starts cannot be split evenly over {G} observation series")
        per = n // G
        pad = (-per) % self.block_threads if G > 1 else 0
        keep = (np.arange(n) // per) * (per + pad) + np.arange(n) % per
        if pad:
            q0 = np.concatenate([np.concatenate([q0[g * per:(g + 1) * per], np.repeat(q0[g * per:g * per + 1], pad, axis=0)]) for g in range(G)])
        if ready is not None:
            ready()
        q, obs = self._in(q0), self._in(obs)
        ssq, grad, jtj = normal(q, obs, fd)
        running = np.isfinite(_host(ssq))
        lam = self._in(np.full(q0.shape[0], _abi.FIT_LAM0))
        status = self._ints(np.where(running, _abi.FIT_RUNNING, _abi.FIT_FAILED))
        iters = self._ints(np.zeros(q0.shape[0]))
        done = 0
        while done < max_iter and running.any():
            k = min(ipl, max_iter - done)
            run(q, obs, lo, hi, ssq, grad, jtj, lam, status, iters, k, fd, ftol)
            running = self._ints_host(status) == _abi.FIT_RUNNING
            done += k
        return self._fit_result(keep, q, ssq, grad, jtj, lam, status, iters, G, self.nout)

    def fit_from_residuals(self, res_fn, q0, lo, hi, fd_rel_step=None, ftol=1e-9, max_iter=100):
        """fit with the caller's residuals: res_fn(points (m, d) float64 on the host) → residuals model - data (m, N), called for
        points strictly inside the box (the trial points and their forward-difference neighbours, parameter p times
        (1 + fd_rel_step)) and for the start points.  d = 1..3, no model needed.  The normal equations are formed on the host;
        the trial points and the decisions are the GPU's (rsf_fit_trial, rsf_fit_decide).  The forward-difference step is relative:
        a coordinate that is exactly 0 has no sensitivity and its start ends STALLED where it is.  → FitResult (one observation group)."""
        q0, lo, hi, d, fd, ftol, max_iter, _ = self._fit_args(q0, lo, hi, (1, 2, 3), fd_rel_step, ftol, max_iter, 1)
        n = q0.shape[0]

        def normal(pts):
            pq = np.repeat(pts[None], d + 1, axis=0)
            for p in range(d):
                pq[p + 1, :, p] = pq[p + 1, :, p] * (1 + fd)
            R = np.asarray(res_fn(pq.reshape(-1, d)), dtype=np.float64)
            if R.ndim != 2 or R.shape[0] != (d + 1) * n:
                raise ValueError(f"res_fn returned shape {R.shape} for {(d + 1) * n} points: (m, N) residuals")
            R = R.reshape(d + 1, n, -1)
            with np.errstate(invalid="ignore", over="ignore"):
                X = np.stack([(R[p + 1] - R[0]) / (pq[p + 1, :, p] * fd)[:, None] for p in range(d)])
                return (R[0] * R[0]).sum(axis=1), np.einsum("pnk,nk->np", X, R[0]), np.einsum("pnk,rnk->npr", X, X), R.shape[2]

        ssq, grad, jtj, n_obs = normal(q0)
        running = np.isfinite(ssq)
        q, ssq, grad, jtj, lam = (self._in(x) for x in (q0, ssq, grad, jtj, np.full(n, _abi.FIT_LAM0)))
        status, iters = self._ints(np.where(running, _abi.FIT_RUNNING, _abi.FIT_FAILED)), self._ints(np.zeros(n))
        done = 0
        while done < max_iter and running.any():
            qt, ok = self.fit_trial(q, grad, jtj, lam, status, lo, hi)
            s_n, g_n, h_n, _ = normal(_host(qt).reshape(n, d))
            self.fit_decide(q, ssq, grad, jtj, lam, status, iters, qt, ok, self._in(s_n), self._in(g_n), self._in(h_n), ftol)
            running = self._ints_host(status) == _abi.FIT_RUNNING
            done += 1
        return self._fit_result(np.arange(n), q, ssq, grad, jtj, lam, status, iters, 1, n_obs)

    # -- Gauss-Newton manifold MALA (include/rsf_mala.h) ----------------------------------------------------------
    @staticmethod
    def _mala_args(q0, lo, hi, dims, n_iter, eps, lam, shape, seed, offset, fd_rel_step, iters_per_launch, keep, thin):
        """The checks Engine.mala and mala_from_residuals share, made before any library call → (q0 (n, d) a fresh host array, lo,
        hi, d, fd, n_iter, eps, lam, shape, seed, offset, iters_per_launch, keep, thin)"""
        q0 = _host(q0).copy()
        if q0.ndim == 1:
            q0 = q0.reshape(-1, 1)
        if q0.ndim != 2 or q0.shape[0] < 1 or q0.shape[1] not in dims:
            raise ValueError(f"q0 has shape {q0.shape}: (n,) or (n, d) start points, d one of {dims}")
        d = int(q0.shape[1])
        lo, hi = _vec(lo, d, "lo"), _vec(hi, d, "hi")
        if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (lo < hi).all()):
            raise ValueError("the box needs finite lo < hi in every parameter")
        if not ((q0 > lo).all() and (q0 < hi).all()):
            raise ValueError("every start point lies strictly inside the box")
        fd = (1e-6 if d == 1 else 1e-4) if fd_rel_step is None else float(fd_rel_step)
        n_iter, eps, lam, ipl, keep, thin = int(n_iter), float(eps), float(lam), int(iters_per_launch), int(keep), int(thin)
        if not (math.isfinite(fd) and fd > 0.0 and math.isfinite(eps) and eps > 0.0 and math.isfinite(lam) and lam >= 0.0):
            raise ValueError("fd_rel_step and eps are finite and > 0, lam is finite and >= 0")
        if shape is not None and not (math.isfinite(float(shape)) and float(shape) > 0.0):
            raise ValueError("shape is finite and > 0")
        if not (n_iter >= 1 and 1 <= ipl <= _abi.MALA_MAX_ITER and 0 <= keep <= n_iter and thin >= 1 and int(seed) >= 0 and int(offset) >= 0):
            raise ValueError(f"n_iter >= 1, iters_per_launch in [1, {_abi.MALA_MAX_ITER}], 0 <= keep <= n_iter, thin >= 1, seed >= 0, offset >= 0")
        return q0, lo, hi, d, fd, n_iter, eps, lam, None if shape is None else float(shape), int(seed), int(offset), ipl, keep, thin

    def _mala_state(self, q, ssq, grad, jtj, accepted=None, outbox=None, stuck=None):
        """The check of a chain state handed to the low-level calls, which read and write it through raw addresses: q (n, d), ssq
        (n,), grad (n, d), jtj (n, d, d) float64 and the counters (n,) int32, each a C-contiguous array of this engine's memory
        space → (n, d)"""
        if getattr(q, "ndim", 0) != 2:
            raise ValueError("q is (n, d)")
        n, d = int(q.shape[0]), int(q.shape[1])
        t = self._torch
        for what, x, shape, dt in (("q", q, (n, d), "float64"), ("ssq", ssq, (n,), "float64"), ("grad", grad, (n, d), "float64"),
                                   ("jtj", jtj, (n, d, d), "float64"), ("accepted", accepted, (n,), "int32"), ("outbox", outbox, (n,), "int32"),
                                   ("stuck", stuck, (n,), "int32")):
            if x is None and dt == "int32":
                continue
            if self.mem == "device":
                good = isinstance(x, t.Tensor) and x.is_cuda and x.is_contiguous() and str(x.dtype) == "torch." + dt
            else:
                good = isinstance(x, np.ndarray) and x.flags["C_CONTIGUOUS"] and x.dtype == np.dtype(dt)
            if not good or tuple(x.shape) != shape:
                raise ValueError(f"{what} must be a C-contiguous {dt} array of shape {shape} in this engine's memory space ({self.mem})")
        return n, d

    def mala_run(self, q, ssq, grad, jtj, data, lo, hi, n_iter, accepted, outbox, stuck, eps=1.0, lam=_abi.FIT_LAM0, shape=None, seed=0,
                 offset=0, iter0=1, fd_rel_step=None, trace=False):
        """rsf_mala_run, the fused hot path: n_iter iterations IN PLACE in q (n, d), ssq, grad, jtj (as fit_normal leaves them) and
        the int32 counters accepted, outbox and stuck, contiguous arrays of this engine's memory space; iteration k uses the draws
        of Philox iteration iter0 + k of chain offset + i.  trace=True → (trace_q (n_iter, n, d), trace_ssq (n_iter, n)), the state
        after each iteration."""
        self._need_model()
        n, d = self._mala_state(q, ssq, grad, jtj, accepted, outbox, stuck)
        data = self._in(data)
        G = int(data.shape[0]) if data.ndim == 2 else 1
        fd = (1e-6 if d == 1 else 1e-4) if fd_rel_step is None else float(fd_rel_step)
        tq, ts = (self._empty((int(n_iter), n, d)), self._empty((int(n_iter), n))) if trace else (None, None)
        _abi.check(self.lib, self.lib.rsf_mala_run(self._ctx, n, d, self._ptr(q), self._ptr(ssq), self._ptr(grad), self._ptr(jtj), self._ptr(data), G,
                                                   _dp(_vec(lo, d, "lo")), _dp(_vec(hi, d, "hi")), fd, float(eps), float(lam),
                                                   float(0.5 * self.nout if shape is None else shape), int(seed), int(offset), int(iter0), int(n_iter),
                                                   self._ptr(accepted), self._ptr(outbox), self._ptr(stuck), self._ptr(tq), self._ptr(ts)))
        return (tq, ts) if trace else None

    def mala_propose(self, q, ssq, grad, jtj, lo, hi, shape, eps=1.0, lam=_abi.FIT_LAM0, seed=0, offset=0, iteration=1):
        """rsf_mala_propose: the proposals of one iteration → (q_new (n, d), inbox (n,) uint8, stuck (n,) uint8).  inbox is 0 for
        a proposal outside the box and for a chain without a proposal, which stuck marks; such a chain's q_new row is its q."""
        n, d = self._mala_state(q, ssq, grad, jtj)
        qn, inb, stk = self._empty((n, d)), self._empty((n,), np.uint8), self._empty((n,), np.uint8)
        _abi.check(self.lib, self.lib.rsf_mala_propose(self._ctx, n, d, self._ptr(q), self._ptr(ssq), self._ptr(grad), self._ptr(jtj),
                                                       _dp(_vec(lo, d, "lo")), _dp(_vec(hi, d, "hi")), float(eps), float(lam), float(shape), int(seed),
                                                       int(offset), int(iteration), self._ptr(qn), self._ptr(inb), self._ptr(stk)))
        return qn, inb, stk

    def mala_accept(self, q, ssq, grad, jtj, lo, hi, q_new, inbox, ssq_new, grad_new, jtj_new, accepted, outbox, stuck, shape, eps=1.0,
                    lam=_abi.FIT_LAM0, seed=0, offset=0, iteration=1):
        """rsf_mala_accept: the decision of one iteration with the caller's normal equations at mala_propose's q_new, IN PLACE in
        q, ssq, grad, jtj and the int32 counters (contiguous arrays of this engine's memory space); q_new (n, d), inbox (n,),
        ssq_new (n,), grad_new (n, d) and jtj_new (n, d, d) are read (the sums where inbox is 1) and may have any layout.  The
        other arguments are mala_propose's."""
        n, d = self._mala_state(q, ssq, grad, jtj, accepted, outbox, stuck)
        q_new, inbox, ssq_new, grad_new, jtj_new = self._in(q_new), self._bytes(inbox), self._in(ssq_new), self._in(grad_new), self._in(jtj_new)
        if (tuple(q_new.shape), tuple(inbox.shape), tuple(ssq_new.shape), tuple(grad_new.shape), tuple(jtj_new.shape)) != ((n, d), (n,), (n,), (n, d), (n, d, d)):
            raise ValueError(f"q_new and grad_new are ({n}, {d}), inbox and ssq_new ({n},), jtj_new ({n}, {d}, {d})")
        _abi.check(self.lib, self.lib.rsf_mala_accept(self._ctx, n, d, self._ptr(q), self._ptr(ssq), self._ptr(grad), self._ptr(jtj),
                                                      _dp(_vec(lo, d, "lo")), _dp(_vec(hi, d, "hi")), float(eps), float(lam), float(shape), int(seed),
                                                      int(offset), int(iteration), self._ptr(q_new), self._ptr(inbox), self._ptr(ssq_new),
                                                      self._ptr(grad_new), self._ptr(jtj_new), self._ptr(accepted), self._ptr(outbox), self._ptr(stuck)))

    def _mala_result(self, sel, q, ssq, grad, jtj, counters, n_iter, kept, keep, thin, shape, seed, offset):
        d = int(q.shape[1])
        tq = np.concatenate([_host(x)[:, sel] for x, _ in kept]) if kept else np.empty((0, sel.size, d))
        ts = np.concatenate([_host(x)[:, sel] for _, x in kept]) if kept else np.empty((0, sel.size))
        rows = np.arange(n_iter - keep, n_iter)[::thin]
        pick = rows - (n_iter - tq.shape[0])  # the kept launches end at the last iteration
        return MalaResult(_host(q)[sel], _host(ssq)[sel], _host(grad)[sel], _host(jtj)[sel], *(self._ints_host(c)[sel].astype(np.int32) for c in counters),
                          n_iter, np.ascontiguousarray(tq[pick]), np.ascontiguousarray(ts[pick]), rows + 1, shape, seed, offset)

    def mala(self, q0, data, lo, hi, n_iter, eps=1.0, lam=_abi.FIT_LAM0, shape=None, seed=0, offset=0, fd_rel_step=None, iters_per_launch=16,
             keep=0, thin=1):
        """Gauss-Newton manifold MALA of the device model (set_model) against `data` over the strict box (lo, hi), target
        pi(q) ~ SSq(q)^-shape (shape: by default nout / 2): q0 (n,) or (n, d) start points inside the box, d = 1 (Dc) or 3 (Dc, a,
        b); data (nout,), or (G, nout) with the chains split evenly over the G series in order.  rsf_fit_normal at q0, then n_iter
        iterations on the GPU (rsf_mala_run, iters_per_launch per launch, one group solve each).  No proposal covariance, no
        adaptation: eps is the step (1: the Gauss-Newton posterior approximation's own scale), lam the damping of the metric.
        Chain i draws from the Philox stream (seed, offset + i), so chains started at one point are independent.  keep: the
        trailing iterations whose states are kept, every thin-th of them → MalaResult.  With G > 1 each series' chains are padded
        to whole workgroups with copies of its first chain (chain j of series g then has stream offset + g (n / G + pad) + j); the
        result holds the caller's chains only."""
        self._need_model()
        q0, lo, hi, d, fd, n_iter, eps, lam, shape, seed, offset, ipl, keep, thin = self._mala_args(
            q0, lo, hi, (1, 3), n_iter, eps, lam, shape, seed, offset, fd_rel_step, iters_per_launch, keep, thin)
        shape = 0.5 * self.nout if shape is None else shape
        obs = _host(data)
        obs = obs.reshape(1, -1) if obs.ndim == 1 else obs
        if obs.ndim != 2 or obs.shape[1] != self.nout:
            raise ValueError(f"data has shape {obs.shape}: (nout,) or (G, nout), the model produces nout = {self.nout} samples")
        n, G = q0.shape[0], obs.shape[0]
        if n % G:
            raise ValueError(f"{n} chains cannot be split evenly over {G} observation series")
        per = n // G
        pad = (-per) % self.block_threads if G > 1 else 0
        sel = (np.arange(n) // per) * (per + pad) + np.arange(n) % per
        if pad:
            q0 = np.concatenate([np.concatenate([q0[g * per:(g + 1) * per], np.repeat(q0[g * per:g * per + 1], pad, axis=0)]) for g in range(G)])
        q, obs = self._in(q0), self._in(obs)
        ssq, grad, jtj = self.fit_normal(q, obs, fd)
        counters = [self._ints(np.zeros(q0.shape[0])) for _ in range(3)]
        kept, done = [], 0
        while done < n_iter:
            k = min(ipl, n_iter - done)
            tr = self.mala_run(q, ssq, grad, jtj, obs, lo, hi, k, *counters, eps=eps, lam=lam, shape=shape, seed=seed, offset=offset, iter0=done + 1,
                               fd_rel_step=fd, trace=done + k > n_iter - keep)
            if tr is not None:
                kept.append(tr)
            done += k
        return self._mala_result(sel, q, ssq, grad, jtj, counters, n_iter, kept, keep, thin, shape, seed, offset)

    def mala_from_residuals(self, res_fn, q0, lo, hi, n_iter, shape, eps=1.0, lam=_abi.FIT_LAM0, seed=0, offset=0, fd_rel_step=None, keep=0, thin=1,
                            normal_fn=None):
        """mala with the caller's residuals: res_fn(points (m, d) float64 on the host) → residuals model - data (m, N), called for
        the start points, the proposals inside the box and their forward-difference neighbours (parameter p times
        (1 + fd_rel_step)), exactly as fit_from_residuals calls it.  d = 1..3, no model needed; shape has no default.  The normal
        equations are formed on the host, the proposals and the decisions are the GPU's (rsf_mala_propose, rsf_mala_accept).
        normal_fn(points (n, d)) → (ssq (n,), grad (n, d), jtj (n, d, d)), if given, replaces res_fn and its forward differences
        (any deterministic function of the point with a positive definite jtj is a valid metric).  → MalaResult."""
        if shape is None:
            raise ValueError("shape is finite and > 0")
        q0, lo, hi, d, fd, n_iter, eps, lam, shape, seed, offset, _, keep, thin = self._mala_args(
            q0, lo, hi, (1, 2, 3), n_iter, eps, lam, shape, seed, offset, fd_rel_step, 1, keep, thin)
        if (res_fn is None) == (normal_fn is None):
            raise ValueError("one of res_fn and normal_fn")
        n = q0.shape[0]

        def normal(pts):
            if normal_fn is not None:
                s, g, h = (np.ascontiguousarray(x, dtype=np.float64) for x in normal_fn(pts))
                if (s.shape, g.shape, h.shape) != ((n,), (n, d), (n, d, d)):
                    raise ValueError(f"normal_fn returned shapes {s.shape}, {g.shape}, {h.shape} for {n} points")
                return s, g, h
            pq = np.repeat(pts[None], d + 1, axis=0)
            for p in range(d):
                pq[p + 1, :, p] = pq[p + 1, :, p] * (1 + fd)
            R = np.asarray(res_fn(pq.reshape(-1, d)), dtype=np.float64)
            if R.ndim != 2 or R.shape[0] != (d + 1) * n:
                raise ValueError(f"res_fn returned shape {R.shape} for {(d + 1) * n} points: (m, N) residuals")
            R = R.reshape(d + 1, n, -1)
            with np.errstate(invalid="ignore", over="ignore"):
                X = np.stack([(R[p + 1] - R[0]) / (pq[p + 1, :, p] * fd)[:, None] for p in range(d)])
                return (R[0] * R[0]).sum(axis=1), np.einsum("pnk,nk->np", X, R[0]), np.einsum("pnk,rnk->npr", X, X)

        q, ssq, grad, jtj = (self._in(x) for x in (q0, *normal(q0)))
        counters = [self._ints(np.zeros(n)) for _ in range(3)]
        kept = []
        for it in range(1, n_iter + 1):
            kw = dict(shape=shape, eps=eps, lam=lam, seed=seed, offset=offset, iteration=it)
            qn, inb, _ = self.mala_propose(q, ssq, grad, jtj, lo, hi, **kw)
            s_n, g_n, h_n = normal(_host(qn).reshape(n, d))
            self.mala_accept(q, ssq, grad, jtj, lo, hi, qn, inb, s_n, g_n, h_n, *counters, **kw)
            if it > n_iter - keep:
                kept.append((_host(q).copy()[None], _host(ssq).copy()[None]))
        return self._mala_result(np.arange(n), q, ssq, grad, jtj, counters, n_iter, kept, keep, thin, shape, seed, offset)

    # -- the affine-invariant stretch move in island ensembles (include/rsf_ensemble.h) ------------------------------
    @property
    def island_size(self):
        """walkers per island of the ensemble sampler: twice the workgroup's threads"""
        return 2 * self.block_threads

    @staticmethod
    def _ens_mask(log_coords, d):
        """log_coords: None (no parameter), an int bit mask, or d truth values → the bit mask (bit p: parameter p moves as log q_p)"""
        if log_coords is None:
            return 0
        if isinstance(log_coords, (int, np.integer)) and not isinstance(log_coords, (bool, np.bool_)):
            mask = int(log_coords)
        else:
            flags = np.atleast_1d(np.asarray(log_coords)).astype(bool)
            if flags.shape != (d,):
                raise ValueError(f"log_coords holds {flags.size} flags for d = {d} parameters")
            mask = sum(1 << p for p in range(d) if flags[p])
        if mask < 0 or mask >> d:
            raise ValueError(f"log_coords has a bit at or beyond d = {d}")
        return mask

    def _ens_args(self, q0, lo, hi, dims, n_iter, a, log_coords, shape, seed, offset, iters_per_launch, keep, thin):
        """The checks Engine.ensemble and ensemble_from_ssq share, made before any library call → (q0 (n, d) a fresh host array, lo,
        hi, d, n_iter, a, logmask, shape, seed, offset, iters_per_launch, keep, thin)"""
        q0 = _host(q0).copy()
        if q0.ndim == 1:
            q0 = q0.reshape(-1, 1)
        if q0.ndim != 2 or q0.shape[0] < 1 or q0.shape[1] not in dims:
            raise ValueError(f"q0 has shape {q0.shape}: (n,) or (n, d) walkers, d one of {dims}")
        n, d = int(q0.shape[0]), int(q0.shape[1])
        if n % self.island_size:
            raise ValueError(f"{n} walkers are not whole islands of {self.island_size} (twice this engine's workgroup size)")
        lo, hi = _vec(lo, d, "lo"), _vec(hi, d, "hi")
        if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (lo < hi).all()):
            raise ValueError("the box needs finite lo < hi in every parameter")
        mask = self._ens_mask(log_coords, d)
        if any((mask >> p) & 1 and lo[p] < 0.0 for p in range(d)):
            raise ValueError("a parameter that moves in log coordinates needs lo >= 0")
        if not ((q0 > lo).all() and (q0 < hi).all()):
            raise ValueError("stuck start: every walker starts strictly inside the box")
        n_iter, a, ipl, thin = int(n_iter), float(a), int(iters_per_launch), int(thin)
        keep = n_iter if keep is None else int(keep)
        if not (math.isfinite(a) and a > 1.0):
            raise ValueError("a is finite and > 1")
        if shape is not None and not (math.isfinite(float(shape)) and float(shape) > 0.0):
            raise ValueError("shape is finite and > 0")
        if not (n_iter >= 1 and 1 <= ipl <= _abi.ENSEMBLE_MAX_ITER and 0 <= keep <= n_iter and thin >= 1 and int(seed) >= 0 and int(offset) >= 0):
            raise ValueError(f"n_iter >= 1, iters_per_launch in [1, {_abi.ENSEMBLE_MAX_ITER}], 0 <= keep <= n_iter, thin >= 1, seed >= 0, offset >= 0")
        return q0, lo, hi, d, n_iter, a, mask, None if shape is None else float(shape), int(seed), int(offset), ipl, keep, thin

    def _ens_state(self, q, l, accepted=None, outbox=None, stuck=None):
        """The check of a walker state handed to the low-level calls, which read and write it through raw addresses: q (n, d) and
        l (n,) float64 and the counters (n,) int32, each a C-contiguous array of this engine's memory space → (n, d)"""
        if getattr(q, "ndim", 0) != 2:
            raise ValueError("q is (n, d)")
        n, d = int(q.shape[0]), int(q.shape[1])
        t = self._torch
        for what, x, shape, dt in (("q", q, (n, d), "float64"), ("l", l, (n,), "float64"), ("accepted", accepted, (n,), "int32"),
                                   ("outbox", outbox, (n,), "int32"), ("stuck", stuck, (n,), "int32")):
            if x is None and dt == "int32":
                continue
            if self.mem == "device":
                good = isinstance(x, t.Tensor) and x.is_cuda and x.is_contiguous() and str(x.dtype) == "torch." + dt
            else:
                good = isinstance(x, np.ndarray) and x.flags["C_CONTIGUOUS"] and x.dtype == np.dtype(dt)
            if not good or tuple(x.shape) != shape:
                raise ValueError(f"{what} must be a C-contiguous {dt} array of shape {shape} in this engine's memory space ({self.mem})")
        return n, d

    def ensemble_run(self, q, l, data, lo, hi, n_iter, accepted, outbox, stuck, a=2.0, log_coords=None, shape=None, seed=0, offset=0, iter0=1,
                     trace=False):
        """rsf_ensemble_run, the fused hot path: n_iter iterations (two half-steps each) IN PLACE in q (n, d), l (n,) and the int32
        counters accepted, outbox and stuck, contiguous arrays of this engine's memory space; n is a whole number of islands
        (island_size walkers each), iteration k uses the draws of Philox iteration iter0 + k of particle offset + j.  data (nout,)
        or (G, nout), the walkers split evenly over the series in whole islands.  trace=True → (trace_q (n_iter, n, d), trace_l
        (n_iter, n)), the state after each iteration."""
        self._need_model()
        n, d = self._ens_state(q, l, accepted, outbox, stuck)
        data = self._in(data)
        G = int(data.shape[0]) if data.ndim == 2 else 1
        tq, tl = (self._empty((int(n_iter), n, d)), self._empty((int(n_iter), n))) if trace else (None, None)
        _abi.check(self.lib, self.lib.rsf_ensemble_run(self._ctx, n, d, self._ptr(q), self._ptr(l), self._ptr(data), G, _dp(_vec(lo, d, "lo")),
                                                       _dp(_vec(hi, d, "hi")), float(a), self._ens_mask(log_coords, d),
                                                       float(0.5 * self.nout if shape is None else shape), int(seed), int(offset), int(iter0),
                                                       int(n_iter), self._ptr(accepted), self._ptr(outbox), self._ptr(stuck), self._ptr(tq),
                                                       self._ptr(tl)))
        return (tq, tl) if trace else None

    def ensemble_propose(self, q, l, lo, hi, half, a=2.0, log_coords=None, seed=0, offset=0, iteration=1):
        """rsf_ensemble_propose: the proposals of the walkers of half `half` (0 or 1) of every island in one half-step → (q_new
        (n, d), inbox (n,) uint8, logz_jac (n,)).  inbox is 0 for a proposal outside the box and for a stuck walker, whose q_new
        row is its q; the rows of the other half hold q, 0 and 0."""
        n, d = self._ens_state(q, l)
        qn = q.clone() if hasattr(q, "clone") else q.copy()
        inb, lj = self._bytes(np.zeros(n, dtype=np.uint8)), self._in(np.zeros(n))
        _abi.check(self.lib, self.lib.rsf_ensemble_propose(self._ctx, n, d, self._ptr(q), self._ptr(l), _dp(_vec(lo, d, "lo")), _dp(_vec(hi, d, "hi")),
                                                           float(a), self._ens_mask(log_coords, d), int(seed), int(offset), int(iteration), int(half),
                                                           self._ptr(qn), self._ptr(inb), self._ptr(lj)))
        return qn, inb, lj

    def ensemble_ssq(self, q_new, inbox, data, half, ssq_new=None):
        """rsf_ensemble_ssq: the solve of one half-step alone → ssq_new (n,), SSq of the device model at ensemble_propose's q_new
        (n, d) for the walkers of half `half` whose inbox is 1, in ensemble_run's own arrangement — the one source of SSq with
        which propose / accept reproduce ensemble_run bit for bit.  The other entries are ssq_new's (by default 1)."""
        self._need_model()
        q_new, inbox, data = self._in(q_new), self._bytes(inbox), self._in(data)
        if q_new.ndim != 2 or tuple(inbox.shape) != (int(q_new.shape[0]),):
            raise ValueError("q_new is (n, d), inbox (n,)")
        n, d = int(q_new.shape[0]), int(q_new.shape[1])
        G = int(data.shape[0]) if data.ndim == 2 else 1
        out = self._in(np.ones(n) if ssq_new is None else ssq_new)
        out = out.clone() if hasattr(out, "clone") else out.copy()
        _abi.check(self.lib, self.lib.rsf_ensemble_ssq(self._ctx, n, d, self._ptr(q_new), self._ptr(inbox), self._ptr(data), G, int(half), self._ptr(out)))
        return out

    def ensemble_accept(self, q, l, lo, hi, half, q_new, inbox, logz_jac, ssq_new, accepted, outbox, stuck, shape, seed=0, offset=0, iteration=1):
        """rsf_ensemble_accept: the decision of one half-step with the caller's sums of squares ssq_new (n,), read where inbox is 1,
        at ensemble_propose's q_new, IN PLACE in q, l and the int32 counters (contiguous arrays of this engine's memory space);
        only the rows of half `half` of every island are touched."""
        n, d = self._ens_state(q, l, accepted, outbox, stuck)
        q_new, inbox, logz_jac, ssq_new = self._in(q_new), self._bytes(inbox), self._in(logz_jac), self._in(ssq_new)
        if (tuple(q_new.shape), tuple(inbox.shape), tuple(logz_jac.shape), tuple(ssq_new.shape)) != ((n, d), (n,), (n,), (n,)):
            raise ValueError(f"q_new is ({n}, {d}), inbox, logz_jac and ssq_new ({n},)")
        _abi.check(self.lib, self.lib.rsf_ensemble_accept(self._ctx, n, d, self._ptr(q), self._ptr(l), _dp(_vec(lo, d, "lo")), _dp(_vec(hi, d, "hi")),
                                                          float(shape), int(seed), int(offset), int(iteration), int(half), self._ptr(q_new),
                                                          self._ptr(inbox), self._ptr(logz_jac), self._ptr(ssq_new), self._ptr(accepted),
                                                          self._ptr(outbox), self._ptr(stuck)))

    def _ens_result(self, q, l, counters, n_iter, kept, keep, thin, shape, seed, offset, mask, a):
        n, d = int(q.shape[0]), int(q.shape[1])
        tq = np.concatenate([_host(x) for x, _ in kept]) if kept else np.empty((0, n, d))
        tl = np.concatenate([_host(x) for _, x in kept]) if kept else np.empty((0, n))
        rows = np.arange(n_iter - keep, n_iter)[::thin]
        pick = rows - (n_iter - tq.shape[0])  # the kept launches end at the last iteration
        return EnsembleResult(_host(q), _host(l), *(self._ints_host(c).astype(np.int32) for c in counters), n_iter,
                              np.ascontiguousarray(tq[pick]), np.ascontiguousarray(tl[pick]), rows + 1, self.island_size, shape, seed, offset, mask, a)

    @staticmethod
    def _ens_refuse_stuck(l):
        bad = ~np.isfinite(l)
        if bad.any():
            raise ValueError(f"stuck start: {int(bad.sum())} walkers have no finite target value (first: walker {int(np.flatnonzero(bad)[0])})")

    def ensemble(self, q0, data, lo, hi, n_iter, a=2.0, log_coords=None, shape=None, seed=0, offset=0, iters_per_launch=16, keep=None, thin=1):
        """The affine-invariant ensemble sampler (the stretch move of Goodman & Weare 2010) of the device model (set_model) against
        `data` over the strict box (lo, hi), target pi(q) ~ SSq(q)^-shape (shape: by default nout / 2): q0 (n,) or (n, d) walkers
        inside the box, d = 1 (Dc) or 3 (Dc, a, b), n a whole number of ISLANDS of island_size = 2 x the workgroup size walkers —
        independent ensembles, one per workgroup, whose walkers take their proposals from each other: no proposal covariance, no
        gradient, one forward solve per proposal, stretch scale a > 1 the only constant.  log_coords: d truth values (or a bit
        mask); a marked parameter moves as log q_p, which needs lo_p >= 0 (in (log Dc, log a, b) the ridge Dc a = const is a
        straight line).  data (nout,), or (G, nout) with the walkers split evenly over the G series in order, whole islands each.
        The start's l comes from evidence_logtarget; a walker outside the box or without a finite l is refused (ValueError).
        n_iter iterations on the GPU (rsf_ensemble_run, iters_per_launch per launch).  keep: the trailing iterations whose states
        are kept (None: all), every thin-th of them → EnsembleResult."""
        self._need_model()
        q0, lo, hi, d, n_iter, a, mask, shape, seed, offset, ipl, keep, thin = self._ens_args(
            q0, lo, hi, (1, 3), n_iter, a, log_coords, shape, seed, offset, iters_per_launch, keep, thin)
        shape = 0.5 * self.nout if shape is None else shape
        obs = _host(data)
        obs = obs.reshape(1, -1) if obs.ndim == 1 else obs
        if obs.ndim != 2 or obs.shape[1] != self.nout:
            raise ValueError(f"data has shape {obs.shape}: (nout,) or (G, nout), the model produces nout = {self.nout} samples")
        n, G = q0.shape[0], obs.shape[0]
        if n % (G * self.island_size):
            raise ValueError(f"{n} walkers cannot be split over {G} observation series in whole islands of {self.island_size}")
        per = n // G
        q = self._in(q0)
        l0 = np.concatenate([_host(self.evidence_logtarget(q[g * per:(g + 1) * per], obs[g], lo, hi, np.zeros(per), shape)) for g in range(G)])
        self._ens_refuse_stuck(l0)
        l, obs = self._in(l0), self._in(obs)
        counters = [self._ints(np.zeros(n)) for _ in range(3)]
        kept, done = [], 0
        while done < n_iter:
            k = min(ipl, n_iter - done)
            tr = self.ensemble_run(q, l, obs, lo, hi, k, *counters, a=a, log_coords=mask, shape=shape, seed=seed, offset=offset, iter0=done + 1,
                                   trace=done + k > n_iter - keep)
            if tr is not None:
                kept.append(tr)
            done += k
        return self._ens_result(q, l, counters, n_iter, kept, keep, thin, shape, seed, offset, mask, a)

    def ensemble_from_ssq(self, ssq_fn, q0, lo, hi, n_iter, shape, a=2.0, log_coords=None, seed=0, offset=0, keep=None, thin=1):
        """ensemble with the caller's sum of squares: ssq_fn(points (m, d) float64 on the host) → SSq (m,), called for the start
        and, twice per iteration, for the proposals of one half that lie inside the box.  d = 1..3, no model needed; shape has no
        default.  The start's l is -shape log SSq on the host; the proposals and the decisions are the GPU's
        (rsf_ensemble_propose, rsf_ensemble_accept).  → EnsembleResult."""
        if shape is None:
            raise ValueError("shape is finite and > 0")
        q0, lo, hi, d, n_iter, a, mask, shape, seed, offset, _, keep, thin = self._ens_args(
            q0, lo, hi, (1, 2, 3), n_iter, a, log_coords, shape, seed, offset, 1, keep, thin)
        n = q0.shape[0]

        def ssq_at(pts):
            s = np.asarray(ssq_fn(pts), dtype=np.float64).reshape(-1)
            if s.size != pts.shape[0]:
                raise ValueError(f"ssq_fn returned {s.size} values for {pts.shape[0]} points")
            return s

        s0 = ssq_at(q0)
        with np.errstate(divide="ignore", invalid="ignore"):
            l0 = np.where(np.isfinite(s0) & (s0 > 0), -shape * np.log(s0), -np.inf)
        self._ens_refuse_stuck(l0)
        q, l = self._in(q0), self._in(l0)
        counters = [self._ints(np.zeros(n)) for _ in range(3)]
        kept = []
        for it in range(1, n_iter + 1):
            for half in (0, 1):
                kw = dict(seed=seed, offset=offset, iteration=it)
                qn, inb, lj = self.ensemble_propose(q, l, lo, hi, half, a=a, log_coords=mask, **kw)
                inside = np.asarray(inb.cpu() if hasattr(inb, "cpu") else inb).astype(bool)
                s_n = np.ones(n)
                if inside.any():
                    s_n[inside] = ssq_at(_host(qn)[inside])
                self.ensemble_accept(q, l, lo, hi, half, qn, inb, lj, s_n, *counters, shape=shape, **kw)
            if it > n_iter - keep:
                kept.append((_host(q).copy()[None], _host(l).copy()[None]))
        return self._ens_result(q, l, counters, n_iter, kept, keep, thin, shape, seed, offset, mask, a)

    # -- two-stage delayed-rejection Metropolis (include/rsf_dr.h) ------------------------------
    @staticmethod
    def _dr_factors(chol, d, G=None):
        """chol: (d, d), or (G, d, d) lower triangular factors (a scalar or (G,) values at d = 1) → (G, d, d) float64; every entry
        finite, nothing above the diagonal, every diagonal entry > 0"""
        L = np.asarray(chol, dtype=np.float64)
        if d == 1 and L.ndim <= 1:
            L = L.reshape(-1, 1, 1)
        if L.ndim == 2:
            L = L[None]
        if L.ndim != 3 or L.shape[1:] != (d, d) or L.shape[0] < 1:
            raise ValueError(f"chol has shape {np.shape(chol)}: ({d}, {d}) or (G, {d}, {d})")
        if G is not None and L.shape[0] != G:
            L = np.broadcast_to(L, (G, d, d)) if L.shape[0] == 1 else L
            if L.shape[0] != G:
                raise ValueError(f"chol holds {L.shape[0]} factors for {G} groups")
        if not (np.isfinite(L).all() and (np.triu(L, 1) == 0.0).all() and (np.diagonal(L, axis1=1, axis2=2) > 0.0).all()):
            raise ValueError("chol is not a lower triangular factor with a positive finite diagonal")
        return np.ascontiguousarray(L)

    @staticmethod
    def _dr_pack(L):
        """(G, d, d) factors → (G, d (d + 1) / 2) row-major lower triangles, rsf_dr_run's layout"""
        d = L.shape[1]
        r, c = np.tril_indices(d)
        return np.ascontiguousarray(L[:, r, c])

    def _dr_state(self, q, l, counters=()):
        """The check of a chain state handed to the low-level calls, which read and write it through raw addresses: q (n, d) and
        l (n,) float64 and the five counters (n,) int32, each a C-contiguous array of this engine's memory space → (n, d)"""
        if getattr(q, "ndim", 0) != 2:
            raise ValueError("q is (n, d)")
        n, d = int(q.shape[0]), int(q.shape[1])
        names = ("accepted1", "accepted2", "outbox1", "outbox2", "stuck")
        if len(counters) not in (0, 5):
            raise ValueError("the counters are accepted1, accepted2, outbox1, outbox2 and stuck")
        t = self._torch
        for what, x, shape, dt in [("q", q, (n, d), "float64"), ("l", l, (n,), "float64")] + [(k, c, (n,), "int32") for k, c in zip(names, counters)]:
            if self.mem == "device":
                good = isinstance(x, t.Tensor) and x.is_cuda and x.is_contiguous() and str(x.dtype) == "torch." + dt
            else:
                good = isinstance(x, np.ndarray) and x.flags["C_CONTIGUOUS"] and x.dtype == np.dtype(dt)
            if not good or tuple(x.shape) != shape:
                raise ValueError(f"{what} must be a C-contiguous {dt} array of shape {shape} in this engine's memory space ({self.mem})")
        return n, d

    def dr_run(self, q, l, data, lo, hi, chol, n_iter, counters, gamma=0.2, stages=2, shape=None, seed=0, offset=0, iter0=1, trace=False):
        """rsf_dr_run, the fused hot path: n_iter iterations IN PLACE in q (n, d), l (n,) and the five int32 counters (accepted1,
        accepted2, outbox1, outbox2, stuck), contiguous arrays of this engine's memory space; iteration k uses the draws of Philox
        iteration iter0 + k of particle offset + j.  data (nout,) or (G, nout) and chol (d, d) or (G, d, d): the chains split
        evenly over the groups in whole workgroups.  trace=True → (trace_q (n_iter, n, d), trace_l (n_iter, n)), the state after
        each iteration."""
        self._need_model()
        n, d = self._dr_state(q, l, counters)
        data = self._in(data)
        G = int(data.shape[0]) if data.ndim == 2 else 1
        tri = self._dr_pack(self._dr_factors(chol, d, G))
        tq, tl = (self._empty((int(n_iter), n, d)), self._empty((int(n_iter), n))) if trace else (None, None)
        _abi.check(self.lib, self.lib.rsf_dr_run(self._ctx, n, d, self._ptr(q), self._ptr(l), self._ptr(data), G, _dp(_vec(lo, d, "lo")),
                                                 _dp(_vec(hi, d, "hi")), _dp(tri), float(gamma), int(stages),
                                                 float(0.5 * self.nout if shape is None else shape), int(seed), int(offset), int(iter0), int(n_iter),
                                                 *(self._ptr(c) for c in counters), self._ptr(tq), self._ptr(tl)))
        return (tq, tl) if trace else None

    def dr_propose(self, q, l, lo, hi, chol, stage, gamma=0.2, pending=None, seed=0, offset=0, iteration=1):
        """rsf_dr_propose: the proposals of one stage (1 or 2) of one iteration → (y (n, d), mask (n,) uint8).  Stage 1: every chain
        inside the box with a finite l proposes y1; stage 2: the chains whose `pending` byte (dr_accept's of stage 1) is 1 propose
        y2.  mask is 1 for a proposal inside the box; a chain that does not propose has y = q and mask 0.  chol (d, d), or
        (G, d, d) with the chains split evenly over the G factors."""
        return self._dr_propose(self.lib.rsf_dr_propose, q, l, lo, hi, chol, stage, gamma, pending, seed, offset, iteration)

    def _dr_propose(self, fn, q, l, lo, hi, chol, stage, gamma, pending, seed, offset, iteration):
        """dr_propose through the entry point fn: rsf_dr_propose, or rsf_kstiff_dr_propose (kstiff_dr_propose)"""
        n, d = self._dr_state(q, l)
        L = self._dr_factors(chol, d)
        y, mask = self._empty((n, d)), self._bytes(np.zeros(n, dtype=np.uint8))
        pend = None if pending is None else self._bytes(pending)
        _abi.check(self.lib, fn(self._ctx, n, d, self._ptr(q), self._ptr(l), int(L.shape[0]), _dp(_vec(lo, d, "lo")), _dp(_vec(hi, d, "hi")),
                                _dp(self._dr_pack(L)), float(gamma), int(stage), int(seed), int(offset), int(iteration), self._ptr(pend), self._ptr(y),
                                self._ptr(mask)))
        return y, mask

    def dr_ssq(self, y, mask, data, ssq=None):
        """rsf_dr_ssq: the solve of one stage alone → ssq (n,), SSq of the device model at dr_propose's y (n, d) for the chains
        whose mask is 1, in dr_run's own arrangement — the one source of SSq with which propose / accept reproduce dr_run bit for
        bit.  The other entries are ssq's (by default 1)."""
        self._need_model()
        y, mask, data = self._in(y), self._bytes(mask), self._in(data)
        if y.ndim != 2 or tuple(mask.shape) != (int(y.shape[0]),):
            raise ValueError("y is (n, d), mask (n,)")
        n, d = int(y.shape[0]), int(y.shape[1])
        G = int(data.shape[0]) if data.ndim == 2 else 1
        out = self._in(np.ones(n) if ssq is None else ssq)
        out = out.clone() if hasattr(out, "clone") else out.copy()
        _abi.check(self.lib, self.lib.rsf_dr_ssq(self._ctx, n, d, self._ptr(y), self._ptr(mask), self._ptr(data), G, self._ptr(out)))
        return out

    def dr_accept(self, q, l, lo, hi, stage, y, mask, ssq, counters, shape, gamma=0.2, l1=None, pending=None, seed=0, offset=0, iteration=1):
        """rsf_dr_accept: the decision of one stage with the caller's sums of squares ssq (n,), read where mask is 1, at dr_propose's
        y, IN PLACE in q, l and the five int32 counters.  Stage 1 → (l1 (n,), pending (n,) uint8): l(y1) (-inf outside the box) and
        1 for the chains that go on to stage 2, which stage 2 takes back."""
        return self._dr_accept(self.lib.rsf_dr_accept, q, l, lo, hi, stage, y, mask, ssq, counters, shape, gamma, l1, pending, seed, offset, iteration)

    def _dr_accept(self, fn, q, l, lo, hi, stage, y, mask, ssq, counters, shape, gamma, l1, pending, seed, offset, iteration):
        """dr_accept through the entry point fn: rsf_dr_accept, or rsf_kstiff_dr_accept (kstiff_dr_accept)"""
        n, d = self._dr_state(q, l, counters)
        y, mask, ssq = self._in(y), self._bytes(mask), self._in(ssq)
        if (tuple(y.shape), tuple(mask.shape), tuple(ssq.shape)) != ((n, d), (n,), (n,)):
            raise ValueError(f"y is ({n}, {d}), mask and ssq ({n},)")
        if int(stage) == 1:
            l1, pending = self._empty((n,)), self._bytes(np.zeros(n, dtype=np.uint8))
        else:
            if l1 is None or pending is None:
                raise ValueError("stage 2 takes l1 and pending of stage 1's dr_accept")
            l1, pending = self._in(l1), self._bytes(pending)
            if (tuple(l1.shape), tuple(pending.shape)) != ((n,), (n,)):
                raise ValueError(f"l1 and pending are ({n},)")
        _abi.check(self.lib, fn(self._ctx, n, d, self._ptr(q), self._ptr(l), _dp(_vec(lo, d, "lo")), _dp(_vec(hi, d, "hi")), float(gamma), int(stage),
                                float(shape), int(seed), int(offset), int(iteration), self._ptr(y), self._ptr(mask), self._ptr(ssq), self._ptr(l1),
                                self._ptr(pending), *(self._ptr(c) for c in counters)))
        return l1, pending

    def _dr_args(self, q0, lo, hi, chol, dims, n_iter, gamma, stages, shape, seed, offset, iters_per_launch, keep, thin, adapt_launches, iter0):
        """The checks Engine.dr and dr_from_ssq share, made before any library call → (q0 (n, d) a fresh host array, lo, hi, d,
        chol (G or 1, d, d), n_iter, gamma, stages, shape, seed, offset, iters_per_launch, keep, thin, adapt_launches, iter0)"""
        q0 = _host(q0).copy()
        if q0.ndim == 1:
            q0 = q0.reshape(-1, 1)
        if q0.ndim != 2 or q0.shape[0] < 1 or q0.shape[1] not in dims:
            raise ValueError(f"q0 has shape {q0.shape}: (n,) or (n, d) chains, d one of {dims}")
        d = int(q0.shape[1])
        lo, hi = _vec(lo, d, "lo"), _vec(hi, d, "hi")
        if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (lo < hi).all()):
            raise ValueError("the box needs finite lo < hi in every parameter")
        if not ((q0 > lo).all() and (q0 < hi).all()):
            raise ValueError("stuck start: every chain starts strictly inside the box")
        L = self._dr_factors(chol, d)
        n_iter, gamma, stages, ipl, thin, adapt, iter0 = int(n_iter), float(gamma), int(stages), int(iters_per_launch), int(thin), int(adapt_launches), int(iter0)
        keep = n_iter if keep is None else int(keep)
        if not (math.isfinite(gamma) and 0.0 < gamma <= 1.0):
            raise ValueError("gamma lies in (0, 1]")
        if stages not in (1, 2):
            raise ValueError("stages is 1 or 2")
        if shape is not None and not (math.isfinite(float(shape)) and float(shape) > 0.0):
            raise ValueError("shape is finite and > 0")
        if not (n_iter >= 1 and 1 <= ipl <= _abi.DR_MAX_ITER and 0 <= keep <= n_iter and thin >= 1 and int(seed) >= 0 and int(offset) >= 0
                and adapt >= 0 and iter0 >= 1 and iter0 + n_iter <= 2 ** 32):
            raise ValueError(f"n_iter >= 1, iters_per_launch in [1, {_abi.DR_MAX_ITER}], 0 <= keep <= n_iter, thin >= 1, seed >= 0, offset >= 0, "
                             "adapt_launches >= 0, iter0 >= 1 and every iteration below 2^32")
        return q0, lo, hi, d, L, n_iter, gamma, stages, None if shape is None else float(shape), int(seed), int(offset), ipl, keep, thin, adapt, iter0

    def dr_adapted_factor(self, states, lo, hi, old):
        """The burn-in adaptation of one group: states (m, d), every state traced so far pooled over chains and iterations →
        chol((2.38^2 / d) cov + diag((1e-6 (hi - lo))^2)), cov by pool_joint (ddof 1, as np.cov); `old` where the matrix has no
        Cholesky factor (or cov is not finite)."""
        d = int(states.shape[-1])
        cov = self.pool_joint(states)["cov"]
        M = (2.38 ** 2 / d) * cov + np.diag((1e-6 * (_vec(hi, d, "hi") - _vec(lo, d, "lo"))) ** 2)
        try:
            if not np.isfinite(M).all():
                raise np.linalg.LinAlgError
            return np.linalg.cholesky(M)
        except np.linalg.LinAlgError:
            return np.asarray(old, dtype=np.float64)

    def _dr_result(self, q, l, counters, n_iter, kept, keep, thin, L, gamma, stages, shape, seed, offset, iter0):
        n, d = int(q.shape[0]), int(q.shape[1])
        tq = np.concatenate([_host(x) for x, _ in kept]) if kept else np.empty((0, n, d))
        tl = np.concatenate([_host(x) for _, x in kept]) if kept else np.empty((0, n))
        rows = np.arange(n_iter - keep, n_iter)[::thin]
        pick = rows - (n_iter - tq.shape[0])  # the kept launches end at the last iteration
        return DrResult(_host(q), _host(l), [self._ints_host(c).astype(np.int32) for c in counters], n_iter, np.ascontiguousarray(tq[pick]),
                        np.ascontiguousarray(tl[pick]), rows + iter0, L.copy(), gamma, stages, shape, seed, offset, iter0)

    def dr(self, q0, data, lo, hi, chol, n_iter, gamma=0.2, stages=2, shape=None, seed=0, offset=0, iters_per_launch=16, keep=None, thin=1,
           adapt_launches=0, iter0=1, l0=None):
        """Two-stage delayed-rejection Metropolis (Mira 2001) of the device model (set_model) against `data` over the strict box
        (lo, hi), target pi(q) ~ SSq(q)^-shape (shape: by default nout / 2): q0 (n,) or (n, d) chains inside the box, d = 1 (Dc) or
        3 (Dc, a, b).  A chain proposes q + L z; when that is rejected — a proposal outside the box is, without a solve — it
        proposes q + gamma L z' in the same iteration, accepted with the probability that keeps pi exact.  No gradient, no fit, no
        other chain.  stages=1 is the plain random walk.  data (nout,), or (G, nout) with the chains split evenly over the G series
        in order (whole workgroups each); chol (d, d) lower triangular, or (G, d, d), one factor per series.
        The start's l comes from evidence_logtarget; a chain outside the box or without a finite l is refused (ValueError).
        n_iter iterations on the GPU (rsf_dr_run, iters_per_launch per launch) at the Philox iterations iter0 .. iter0 + n_iter - 1.
        adapt_launches = k: after each of the first k launches every group's factor becomes dr_adapted_factor of every state traced
        so far; then it is frozen.  Iterations of an adapting launch are burn-in: a sample of pi is what the launches after them
        give (MCMC.sample_dr adapts inside its burn-in only).  l0 (n,): the chains' l at q0, for a run that continues an earlier one
        bit for bit (DrResult.q, .l and .chol, iter0 = the next Philox iteration); by default evidence_logtarget's.  keep: the
        trailing iterations whose states are kept (None: all), every thin-th of them → DrResult."""
        self._need_model()
        start_l = lambda q, obs, lo, hi, shape: _host(self.evidence_logtarget(q, obs, lo, hi, np.zeros(int(q.shape[0])), shape))
        return self._dr_drive(self.dr_run, start_l, q0, data, lo, hi, chol, n_iter, gamma, stages, shape, seed, offset, iters_per_launch, keep, thin,
                              adapt_launches, iter0, l0)

    def _dr_drive(self, run, start_l, q0, data, lo, hi, chol, n_iter, gamma, stages, shape, seed, offset, iters_per_launch, keep, thin, adapt_launches,
                  iter0, l0, ready=None, dims=(1, 3)):
        """What Engine.dr, Engine.law_dr and Engine.kstiff_dr share, everything but the solve: the checks, the groups, the launches
        of `run` (dr_run's signature) with the burn-in adaptation between them, the kept traces.  start_l(q (per, d) in this
        engine's memory space, obs (nout,) on the host, lo, hi, shape) → the start's l of one group on the host; ready(): called
        after the argument checks and before the first library call; dims: the chain dimensions `run` takes."""
        q0, lo, hi, d, L, n_iter, gamma, stages, shape, seed, offset, ipl, keep, thin, adapt, iter0 = self._dr_args(
            q0, lo, hi, chol, dims, n_iter, gamma, stages, shape, seed, offset, iters_per_launch, keep, thin, adapt_launches, iter0)
        shape = 0.5 * self.nout if shape is None else shape
        obs = _host(data)
        obs = obs.reshape(1, -1) if obs.ndim == 1 else obs
        if obs.ndim != 2 or obs.shape[1] != self.nout or not 1 <= obs.shape[0] <= _abi.DR_MAX_GROUPS:
            raise ValueError(f"data has shape {obs.shape}: (nout,) or (G, nout), G <= {_abi.DR_MAX_GROUPS}; the model produces nout = {self.nout} samples")
        n, G = q0.shape[0], obs.shape[0]
        if G > 1 and n % (G * self.block_threads):
            raise ValueError(f"{n} chains cannot be split over {G} observation series in whole workgroups of {self.block_threads}")
        L = self._dr_factors(L, d, G).copy()
        per = n // G
        if ready is not None:
            ready()
        q = self._in(q0)
        if l0 is None:
            l0 = np.concatenate([start_l(q[g * per:(g + 1) * per], obs[g], lo, hi, shape) for g in range(G)])
        else:
            l0 = _host(l0).reshape(-1).copy()
            if l0.shape != (n,):
                raise ValueError(f"l0 holds {l0.size} values for {n} chains")
        self._ens_refuse_stuck(l0)
        l, obs = self._in(l0), self._in(obs)
        counters = [self._ints(np.zeros(n)) for _ in range(5)]
        kept, seen, done, launch = [], [], 0, 0
        while done < n_iter:
            k = min(ipl, n_iter - done)
            adapting = launch < adapt
            tr = run(q, l, obs, lo, hi, L, k, counters, gamma=gamma, stages=stages, shape=shape, seed=seed, offset=offset, iter0=iter0 + done,
                     trace=adapting or done + k > n_iter - keep)
            if adapting:
                seen.append(tr[0])
                for g in range(G):
                    L[g] = self.dr_adapted_factor(self._dr_pool(seen, g * per, (g + 1) * per), lo, hi, L[g])
            if done + k > n_iter - keep:
                kept.append(tr)
            done += k
            launch += 1
        return self._dr_result(q, l, counters, n_iter, kept, keep, thin, L, gamma, stages, shape, seed, offset, iter0)

    @staticmethod
    def _dr_pool(traces, first, last):
        """the rows first .. last - 1 of every traced iteration (k, n, d) → (m, d), contiguous, in the traces' memory space"""
        parts = [t[:, first:last].reshape(-1, t.shape[-1]) for t in traces]
        if isinstance(parts[0], np.ndarray):
            return np.concatenate(parts)
        import torch

        return torch.cat(parts).contiguous()

    def dr_from_ssq(self, ssq_fn, q0, lo, hi, chol, n_iter, shape, gamma=0.2, stages=2, seed=0, offset=0, keep=None, thin=1, iter0=1):
        """dr with the caller's sum of squares: ssq_fn(points (m, d) float64 on the host) → SSq (m,), called for the start and, up to
        twice per iteration, for the proposals of one stage that lie inside the box.  d = 1..3, no model needed; shape has no
        default; one factor chol (d, d).  The start's l is -shape log SSq on the host; the proposals and the decisions are the
        GPU's (rsf_dr_propose, rsf_dr_accept).  → DrResult."""
        if shape is None:
            raise ValueError("shape is finite and > 0")
        q0, lo, hi, d, L, n_iter, gamma, stages, shape, seed, offset, _, keep, thin, _, iter0 = self._dr_args(
            q0, lo, hi, chol, (1, 2, 3), n_iter, gamma, stages, shape, seed, offset, 1, keep, thin, 0, iter0)
        if L.shape[0] != 1:
            raise ValueError("dr_from_ssq takes one factor (d, d)")
        n = q0.shape[0]

        def ssq_at(pts):
            s = np.asarray(ssq_fn(pts), dtype=np.float64).reshape(-1)
            if s.size != pts.shape[0]:
                raise ValueError(f"ssq_fn returned {s.size} values for {pts.shape[0]} points")
            return s

        def solved(y, mask):
            inside = np.asarray(mask.cpu() if hasattr(mask, "cpu") else mask).astype(bool)
            s = np.ones(n)
            if inside.any():
                s[inside] = ssq_at(_host(y)[inside])
            return s

        s0 = ssq_at(q0)
        with np.errstate(divide="ignore", invalid="ignore"):
            l0 = np.where(np.isfinite(s0) & (s0 > 0), -shape * np.log(s0), -np.inf)
        self._ens_refuse_stuck(l0)
        q, l = self._in(q0), self._in(l0)
        counters = [self._ints(np.zeros(n)) for _ in range(5)]
        kept = []
        for k in range(n_iter):
            kw = dict(gamma=gamma, seed=seed, offset=offset, iteration=iter0 + k)
            y, mask = self.dr_propose(q, l, lo, hi, L, 1, **kw)
            l1, pend = self.dr_accept(q, l, lo, hi, 1, y, mask, solved(y, mask), counters, shape, **kw)
            if stages == 2:
                y, mask = self.dr_propose(q, l, lo, hi, L, 2, pending=pend, **kw)
                self.dr_accept(q, l, lo, hi, 2, y, mask, solved(y, mask), counters, shape, l1=l1, pending=pend, **kw)
            if k >= n_iter - keep:
                kept.append((_host(q).copy()[None], _host(l).copy()[None]))
        return self._dr_result(q, l, counters, n_iter, kept, keep, thin, L, gamma, stages, shape, seed, offset, iter0)

    # -- delayed rejection under either state law and any observable (include/rsf_law_dr.h) ------------------------------
    def _law_dr_fn(self, name):
        """a function of include/rsf_law_dr.h, which librsf_hip.so alone exports"""
        try:
            return getattr(self.lib, name)
        except AttributeError:
            raise _abi.RsfError(-5, f"{name} is exported by librsf_hip.so only: the {self.lib.rsf_backend().decode()!r} library has no such "
                                    "symbol (include/rsf_law_dr.h)") from None

    @staticmethod
    def _law_codes(law, observable):
        """names or aliases of _abi.LAWS / _abi.OBSERVABLES → their codes, law_observe's checks; integers pass through"""
        if isinstance(law, str):
            if law not in _abi.LAWS:
                raise ValueError(f"law is 'aging' (or 'ageing') or 'slip', not {law!r}")
            law = _abi.LAWS[law]
        if isinstance(observable, str):
            observable = _abi.OBSERVABLES[observable_name(observable)]
        return int(law), int(observable)

    def stiff_dr_run(self, law, observable, stiffness, q, l, data, lo, hi, chol, n_iter, counters, **kw):
        """rsf_stiff_dr_run, the fused hot path of include/rsf_stiff.h: law_dr_run — its arguments, checks and results — with the
        spring's stiffness `stiffness`, a constant independent of Dc."""
        return self.law_dr_run(law, observable, q, l, data, lo, hi, chol, n_iter, counters, stiffness=float(stiffness), **kw)

    def stiff_dr_ssq(self, law, observable, stiffness, y, mask, data, ssq=None):
        """rsf_stiff_dr_ssq: law_dr_ssq with the spring's stiffness `stiffness` → stiff_observe's SSq bit for bit."""
        return self.law_dr_ssq(law, observable, y, mask, data, ssq=ssq, stiffness=float(stiffness))

    def _stiff_args(self, name, stiffness):
        """(the entry point, the arguments between `observable` and the chains) of a law_dr call: rsf_law_dr_* without a stiffness
        in force, rsf_stiff_dr_* and the stiffness with one"""
        k = self._stiffness(stiffness)
        if k is None:
            return self._law_dr_fn("rsf_law_" + name), ()
        return self._stiff_fn("rsf_stiff_" + name), (k,)

    def law_dr_run(self, law, observable, q, l, data, lo, hi, chol, n_iter, counters, gamma=0.2, stages=2, shape=None, seed=0, offset=0, iter0=1,
                   trace=False, stiffness=None):
        """rsf_law_dr_run: dr_run — its arguments, checks and results — with the solve under the state law `law` against `data`,
        series of `observable` (law_observe's names, aliases or integers), under the loading table in use.  stiffness: None, the
        engine's model's; with one in force the launch is rsf_stiff_dr_run."""
        self._need_model(law_aware=True, stiff_aware=True)
        return self._law_dr_run(lambda: self._stiff_args("dr_run", stiffness), law, observable, q, l, data, lo, hi, chol, n_iter, counters, gamma,
                                stages, shape, seed, offset, iter0, trace)

    def _law_dr_run(self, entry, law, observable, q, l, data, lo, hi, chol, n_iter, counters, gamma, stages, shape, seed, offset, iter0, trace):
        """law_dr_run through entry() → (the entry point, the arguments between `observable` and the chains), asked for after the
        argument checks: rsf_law_dr_run (), rsf_stiff_dr_run (stiffness,) or rsf_kstiff_dr_run () (kstiff_dr_run)"""
        law, observable = self._law_codes(law, observable)
        n, d = self._dr_state(q, l, counters)
        data = self._in(data)
        G = int(data.shape[0]) if data.ndim == 2 else 1
        tri = self._dr_pack(self._dr_factors(chol, d, G))
        fn, k = entry()
        tq, tl = (self._empty((int(n_iter), n, d)), self._empty((int(n_iter), n))) if trace else (None, None)
        _abi.check(self.lib, fn(self._ctx, law, observable, *k, n, d, self._ptr(q), self._ptr(l), self._ptr(data), G, _dp(_vec(lo, d, "lo")),
                                _dp(_vec(hi, d, "hi")), _dp(tri), float(gamma), int(stages), float(0.5 * self.nout if shape is None else shape),
                                int(seed), int(offset), int(iter0), int(n_iter), *(self._ptr(c) for c in counters), self._ptr(tq), self._ptr(tl)))
        return (tq, tl) if trace else None

    def law_dr_ssq(self, law, observable, y, mask, data, ssq=None, stiffness=None):
        """rsf_law_dr_ssq: dr_ssq under `law` against `data` of `observable` → ssq (n,), law_observe's SSq bit for bit at dr_propose's
        y (n, d) for the chains whose mask is 1, solved in law_dr_run's arrangement.  The other entries are ssq's (by default 1).
        stiffness: None, the engine's model's; with one in force the launch is rsf_stiff_dr_ssq."""
        self._need_model(law_aware=True, stiff_aware=True)
        return self._law_dr_ssq(lambda: self._stiff_args("dr_ssq", stiffness), law, observable, y, mask, data, ssq)

    def _law_dr_ssq(self, entry, law, observable, y, mask, data, ssq):
        """law_dr_ssq through entry(), as _law_dr_run"""
        law, observable = self._law_codes(law, observable)
        y, mask, data = self._in(y), self._bytes(mask), self._in(data)
        if y.ndim != 2 or tuple(mask.shape) != (int(y.shape[0]),):
            raise ValueError("y is (n, d), mask (n,)")
        n, d = int(y.shape[0]), int(y.shape[1])
        G = int(data.shape[0]) if data.ndim == 2 else 1
        fn, k = entry()
        out = self._in(np.ones(n) if ssq is None else ssq)
        out = out.clone() if hasattr(out, "clone") else out.copy()
        _abi.check(self.lib, fn(self._ctx, law, observable, *k, n, d, self._ptr(y), self._ptr(mask), self._ptr(data), G, self._ptr(out)))
        return out

    def law_gn_factor(self, law, observable, q, data, rel_step=1e-4, stiffness=None):
        """The Gauss-Newton proposal at the point q (d,), d = 1 (Dc) or 3 (Dc, a, b) → (L, cov, ssq): from ONE law_observe call of
        1 + d lanes, q and q + rel_step q_p e_p, the Jacobian J of the series by forward differences; cov = (SSq / nout) (J^T J)^-1,
        the Laplace covariance of the posterior at q, and L = chol((2.38^2 / d) cov), the random walk's factor.  What factor="init"
        is for the tier kernels, without an init kernel and without a fit.  ValueError where a series is not finite or the matrix
        has no Cholesky factor.  stiffness: None, the engine's model's; law_observe's."""
        self._need_model(law_aware=True, stiff_aware=True)
        law, observable = self._law_codes(law, observable)
        q = np.asarray(_host(q), dtype=np.float64).reshape(-1)
        d = q.size
        if d not in (1, 3) or not np.isfinite(q).all() or not (q != 0.0).all() or not (math.isfinite(float(rel_step)) and float(rel_step) > 0.0):
            raise ValueError(f"q has shape {q.shape}: a finite point (Dc,) or (Dc, a, b) without a zero, and rel_step is finite and > 0")
        obs = _host(data).reshape(-1)
        if obs.size != self.nout:
            raise ValueError(f"data has {obs.size} entries, the model produces {self.nout}")
        self._stiff_args("dr_run", stiffness)  # the factor of this family's sampler: a library without it is refused here
        h = float(rel_step) * q
        pts = np.tile(q, (1 + d, 1))
        pts[1:] += np.diag(h)
        ab = [np.ascontiguousarray(pts[:, p]) for p in (1, 2)] if d == 3 else [None, None]
        series = _host(self.law_observe(law, observable, np.ascontiguousarray(pts[:, 0]), ab[0], ab[1], want_series=True, stiffness=stiffness)[1])
        return self._gn_factor("law_gn_factor", q, h, obs, series)

    def _gn_factor(self, name, q, h, obs, series):
        """The rule law_gn_factor and kstiff_gn_factor share: series (nout, 1 + d) at q and at q + h_p e_p, the data obs → (L, cov, ssq)"""
        d = q.size
        if not np.isfinite(series).all():
            raise ValueError(f"{name}: the series at q = {q.tolist()} or beside it is not finite")
        r = series[:, 0] - obs
        ssq = float(r @ r)
        J = (series[:, 1:] - series[:, :1]) / h
        try:
            cov = (ssq / self.nout) * np.linalg.inv(J.T @ J)
            if not np.isfinite(cov).all():
                raise np.linalg.LinAlgError
            L = np.linalg.cholesky((2.38 ** 2 / d) * cov)
        except np.linalg.LinAlgError:
            raise ValueError(f"{name}: (SSq / nout) (J^T J)^-1 at q = {q.tolist()} has no Cholesky factor (a parameter the series "
                             "does not depend on, or a step too small for it)") from None
        return L, cov, ssq

    def law_dr(self, law, observable, q0, data, lo, hi, chol, n_iter, gamma=0.2, stages=2, shape=None, seed=0, offset=0, iters_per_launch=16, keep=None,
               thin=1, adapt_launches=0, iter0=1, l0=None, stiffness=None):
        """Engine.dr — its arguments, groups, adaptation, continuation and result, through the same driver — for the device model
        under the state law `law` against `data`, series of `observable`: the launch is law_dr_run, and the start's l is what
        dr_from_ssq forms, -shape log SSq in NumPy on the host from law_ssq_fn(law, data_g, observable) (-inf where SSq is not
        finite and > 0; such a start is refused).  With adapt_launches = 0 the run is dr_from_ssq(law_ssq_fn(...), ...)'s bit for
        bit, from the first state on.  stiffness: None, the engine's model's; with one in force the launches are rsf_stiff_dr_run's
        and the start's l stiff_observe's."""
        self._need_model(law_aware=True, stiff_aware=True)
        stiffness = self._stiffness(stiffness)
        codes = self._law_codes(law, observable)
        if codes[1] not in _OBSERVABLE_NAMES:
            raise ValueError(f"observable is one of {sorted(_OBSERVABLE_NAMES)} (RSF_OBS_*), not {codes[1]}")

        def start_l(q, obs, lo, hi, shape):
            s = np.asarray(self.law_ssq_fn(codes[0], obs, _OBSERVABLE_NAMES[codes[1]], stiffness=stiffness)(_host(q)), dtype=np.float64).reshape(-1)
            with np.errstate(divide="ignore", invalid="ignore"):
                return np.where(np.isfinite(s) & (s > 0), -shape * np.log(s), -np.inf)

        run = lambda q, l, obs, lo, hi, L, k, counters, **kw: self.law_dr_run(codes[0], codes[1], q, l, obs, lo, hi, L, k, counters,
                                                                              stiffness=stiffness, **kw)
        return self._dr_drive(run, start_l, q0, data, lo, hi, chol, n_iter, gamma, stages, shape, seed, offset, iters_per_launch, keep, thin,
                              adapt_launches, iter0, l0, ready=lambda: self._stiff_args("dr_run", stiffness))

    # -- the stiffness among the parameters: chains over (Dc, k) or (Dc, a, b, k) (include/rsf_kstiff.h) -----------------
    # These calls take the stiffness from the points, its last coordinate, whatever the engine's model's stiffness is.
    def _kstiff_fn(self, name):
        """a function of include/rsf_kstiff.h, which librsf_hip.so alone exports"""
        try:
            return getattr(self.lib, name)
        except AttributeError:
            raise _abi.RsfError(-5, f"{name} is exported by librsf_hip.so only: the {self.lib.rsf_backend().decode()!r} library has no such "
                                    "symbol (include/rsf_kstiff.h)") from None

    def kstiff_observe(self, law, observable, dc, k, a=None, b=None, data=None, want_ssq=False, want_series=True):
        """rsf_kstiff_observe: stiff_observe — its arguments, checks and results — with the stiffness k[C] of each point in place of
        the call's one stiffness; every k[i] is finite and > 0."""
        self._need_model(law_aware=True, stiff_aware=True)
        law, observable = self._law_codes(law, observable)
        dc = self._in(np.atleast_1d(dc) if not hasattr(dc, "data_ptr") else dc)
        k = self._in(np.atleast_1d(k) if not hasattr(k, "data_ptr") else k)
        C = int(dc.shape[0])
        if tuple(k.shape) != (C,):
            raise ValueError(f"k has shape {tuple(k.shape)}: one stiffness per point, ({C},)")
        a, b, data = self._in(a), self._in(b), self._in(data)
        if want_ssq and data is None:
            raise ValueError("want_ssq needs data")
        if data is not None and int(data.shape[0]) != self.nout:
            raise ValueError(f"data has {int(data.shape[0])} entries, the model produces {self.nout}")
        ssq = self._empty((C,)) if want_ssq else None
        series = self._empty((self.nout, C)) if want_series else None
        _abi.check(self.lib, self._kstiff_fn("rsf_kstiff_observe")(self._ctx, law, observable, C, self._ptr(dc), self._ptr(a), self._ptr(b),
                                                                   self._ptr(k), self._ptr(data), self._ptr(ssq), self._ptr(series)))
        return ssq, series

    @staticmethod
    def _kstiff_columns(pts):
        """points (m, 2) of (Dc, k) or (m, 4) of (Dc, a, b, k) on the host → (dc, a, b, k), contiguous columns (a, b None at d = 2)"""
        pts = np.asarray(pts, dtype=np.float64)
        if pts.ndim != 2 or pts.shape[1] not in (2, 4):
            raise ValueError(f"the points have shape {pts.shape}: (m, 2) of (Dc, k) or (m, 4) of (Dc, a, b, k)")
        col = lambda p: np.ascontiguousarray(pts[:, p])
        return (col(0), col(1), col(2), col(3)) if pts.shape[1] == 4 else (col(0), None, None, col(1))

    def kstiff_ssq_fn(self, law, data, observable="acc"):
        """law_ssq_fn with the stiffness among the parameters: points (m, 2) of (Dc, k) or (m, 4) of (Dc, a, b, k) on the host → SSq
        (m,) on the host, solved by kstiff_observe."""
        obs = self._in(data)

        def ssq_fn(pts):
            dc, a, b, k = self._kstiff_columns(pts)
            return _host(self.kstiff_observe(law, observable, dc, k, a, b, data=obs, want_ssq=True, want_series=False)[0])

        return ssq_fn

    def kstiff_dr_run(self, law, observable, q, l, data, lo, hi, chol, n_iter, counters, gamma=0.2, stages=2, shape=None, seed=0, offset=0, iter0=1,
                      trace=False):
        """rsf_kstiff_dr_run, the fused hot path of include/rsf_kstiff.h: law_dr_run — its arguments, checks and results — on chains
        q (n, 2) of (Dc, k) or (n, 4) of (Dc, a, b, k); lo[d - 1] > 0."""
        self._need_model(law_aware=True, stiff_aware=True)
        return self._law_dr_run(lambda: (self._kstiff_fn("rsf_kstiff_dr_run"), ()), law, observable, q, l, data, lo, hi, chol, n_iter, counters, gamma,
                                stages, shape, seed, offset, iter0, trace)

    def kstiff_dr_ssq(self, law, observable, y, mask, data, ssq=None):
        """rsf_kstiff_dr_ssq: law_dr_ssq at points y (n, 2) or (n, 4) with the stiffness last → kstiff_observe's SSq bit for bit."""
        self._need_model(law_aware=True, stiff_aware=True)
        return self._law_dr_ssq(lambda: (self._kstiff_fn("rsf_kstiff_dr_ssq"), ()), law, observable, y, mask, data, ssq)

    def kstiff_dr_propose(self, q, l, lo, hi, chol, stage, gamma=0.2, pending=None, seed=0, offset=0, iteration=1):
        """rsf_kstiff_dr_propose: dr_propose — its arguments and results — at d = 2 or 4 (at d = 2 bit for bit); lo[d - 1] > 0."""
        return self._dr_propose(self._kstiff_fn("rsf_kstiff_dr_propose"), q, l, lo, hi, chol, stage, gamma, pending, seed, offset, iteration)

    def kstiff_dr_accept(self, q, l, lo, hi, stage, y, mask, ssq, counters, shape, gamma=0.2, l1=None, pending=None, seed=0, offset=0, iteration=1):
        """rsf_kstiff_dr_accept: dr_accept — its arguments and results — at d = 2 or 4 (at d = 2 bit for bit); lo[d - 1] > 0."""
        return self._dr_accept(self._kstiff_fn("rsf_kstiff_dr_accept"), q, l, lo, hi, stage, y, mask, ssq, counters, shape, gamma, l1, pending, seed,
                               offset, iteration)

    def kstiff_gn_factor(self, law, observable, q, data, rel_step=1e-4):
        """law_gn_factor's rule at the point q = (Dc, k) or (Dc, a, b, k) → (L, cov, ssq), from ONE kstiff_observe call of 1 + d
        lanes: cov = (SSq / nout) (J^T J)^-1 and L = chol((2.38^2 / d) cov).  Under a hold history the four-parameter matrix is
        nearly singular (MCMC.sample_stiffness)."""
        self._need_model(law_aware=True, stiff_aware=True)
        law, observable = self._law_codes(law, observable)
        q = np.asarray(_host(q), dtype=np.float64).reshape(-1)
        d = q.size
        if d not in (2, 4) or not np.isfinite(q).all() or not (q != 0.0).all() or not (math.isfinite(float(rel_step)) and float(rel_step) > 0.0):
            raise ValueError(f"q has shape {q.shape}: a finite point (Dc, k) or (Dc, a, b, k) without a zero, and rel_step is finite and > 0")
        obs = _host(data).reshape(-1)
        if obs.size != self.nout:
            raise ValueError(f"data has {obs.size} entries, the model produces {self.nout}")
        self._kstiff_fn("rsf_kstiff_dr_run")  # the factor of this family's sampler: a library without it is refused here
        h = float(rel_step) * q
        pts = np.tile(q, (1 + d, 1))
        pts[1:] += np.diag(h)
        dc, a, b, k = self._kstiff_columns(pts)
        return self._gn_factor("kstiff_gn_factor", q, h, obs, _host(self.kstiff_observe(law, observable, dc, k, a, b, want_series=True)[1]))

    def kstiff_dr(self, law, observable, q0, data, lo, hi, chol, n_iter, gamma=0.2, stages=2, shape=None, seed=0, offset=0, iters_per_launch=16,
                  keep=None, thin=1, adapt_launches=0, iter0=1, l0=None):
        """Engine.law_dr — its arguments, groups, adaptation, continuation and DrResult, through the same driver — with the
        stiffness among the parameters: q0 (n, 2) chains over (Dc, k) or (n, 4) over (Dc, a, b, k), lo[d - 1] > 0.  The launch is
        kstiff_dr_run and the start's l is -shape log SSq from kstiff_ssq_fn."""
        self._need_model(law_aware=True, stiff_aware=True)
        codes = self._law_codes(law, observable)
        if codes[1] not in _OBSERVABLE_NAMES:
            raise ValueError(f"observable is one of {sorted(_OBSERVABLE_NAMES)} (RSF_OBS_*), not {codes[1]}")
        if not (np.asarray(_host(lo), dtype=np.float64).reshape(-1)[-1] > 0.0):
            raise ValueError("the box of the stiffness, the last coordinate, lies in k > 0")

        def start_l(q, obs, lo, hi, shape):
            s = np.asarray(self.kstiff_ssq_fn(codes[0], obs, _OBSERVABLE_NAMES[codes[1]])(_host(q)), dtype=np.float64).reshape(-1)
            with np.errstate(divide="ignore", invalid="ignore"):
                return np.where(np.isfinite(s) & (s > 0), -shape * np.log(s), -np.inf)

        run = lambda q, l, obs, lo, hi, L, k, counters, **kw: self.kstiff_dr_run(codes[0], codes[1], q, l, obs, lo, hi, L, k, counters, **kw)
        return self._dr_drive(run, start_l, q0, data, lo, hi, chol, n_iter, gamma, stages, shape, seed, offset, iters_per_launch, keep, thin,
                              adapt_launches, iter0, l0, ready=lambda: self._kstiff_fn("rsf_kstiff_dr_run"), dims=(2, 4))

    # -- Levenberg-Marquardt under either state law and any observable (include/rsf_law_fit.h) ---------------------------
    def _law_fit_fn(self, name):
        """a function of include/rsf_law_fit.h, which librsf_hip.so alone exports"""
        try:
            return getattr(self.lib, name)
        except AttributeError:
            raise _abi.RsfError(-5, f"{name} is exported by librsf_hip.so only: the {self.lib.rsf_backend().decode()!r} library has no such "
                                    "symbol (include/rsf_law_fit.h)") from None

    def _law_fit_data(self, data):
        """data (nout,) or (G, nout) in this engine's memory space → (data, G)"""
        data = self._in(data)
        if data.ndim not in (1, 2) or int(data.shape[-1]) != self.nout:
            raise ValueError(f"data has shape {tuple(data.shape)}: (nout,) or (G, nout), the model produces nout = {self.nout} samples")
        return data, int(data.shape[0]) if data.ndim == 2 else 1

    def law_fit_normal(self, law, observable, q, data, fd_rel_step=None):
        """rsf_law_fit_normal: fit_normal — its arguments and results — with the solve under the state law `law` against `data`,
        series of `observable` (law_observe's names, aliases or integers), under the loading table in use.  ssq is law_observe's SSq
        at q bit for bit."""
        self._need_model(law_aware=True)
        law, observable = self._law_codes(law, observable)
        q = self._in(q)
        if q.ndim == 1:
            q = q.reshape(-1, 1)
        if q.ndim != 2 or int(q.shape[0]) < 1:
            raise ValueError(f"q has shape {tuple(q.shape)}: (n,) or (n, d) points")
        n, d = int(q.shape[0]), int(q.shape[1])
        obs, G = self._law_fit_data(data)
        fd = (1e-6 if d == 1 else 1e-4) if fd_rel_step is None else float(fd_rel_step)
        fn = self._law_fit_fn("rsf_law_fit_normal")
        ssq, grad, jtj = self._empty((n,)), self._empty((n, d)), self._empty((n, d, d))
        _abi.check(self.lib, fn(self._ctx, law, observable, n, d, self._ptr(q), self._ptr(obs), G, fd, self._ptr(ssq), self._ptr(grad), self._ptr(jtj)))
        return ssq, grad, jtj

    def law_fit_run(self, law, observable, q, data, lo, hi, ssq, grad, jtj, lam, status, iters, n_iter, fd_rel_step=None, ftol=1e-9):
        """rsf_law_fit_run, the fused hot path: fit_run — its arguments, IN PLACE in the same seven arrays — with the solve under
        `law` against `data` of `observable`."""
        self._need_model(law_aware=True)
        law, observable = self._law_codes(law, observable)
        n, d = self._fit_state(q, grad, jtj, lam, status, ssq, iters)
        data, G = self._law_fit_data(data)
        fd = (1e-6 if d == 1 else 1e-4) if fd_rel_step is None else float(fd_rel_step)
        lo, hi = _vec(lo, d, "lo"), _vec(hi, d, "hi")
        fn = self._law_fit_fn("rsf_law_fit_run")
        _abi.check(self.lib, fn(self._ctx, law, observable, n, d, self._ptr(q), self._ptr(data), G, _dp(lo), _dp(hi), fd, float(ftol), int(n_iter),
                                self._ptr(ssq), self._ptr(grad), self._ptr(jtj), self._ptr(lam), self._ptr(status), self._ptr(iters)))

    def law_fit(self, law, observable, q0, data, lo, hi, fd_rel_step=None, ftol=1e-9, max_iter=100, iters_per_launch=8):
        """Engine.fit — its arguments, groups, padding, statuses and FitResult, through the same driver — for the device model under
        the state law `law` against `data`, series of `observable`, under the loading table in use: the launches are law_fit_normal
        and law_fit_run, every iteration of every start inside the kernel, only the statuses read between launches.  Any device
        model runs, the default one included (ageing law, acceleration, built-in loading: the plain solve in place of fit's tiers)."""
        self._need_model(law_aware=True)
        codes = self._law_codes(law, observable)
        if codes[0] not in (_abi.LAW_AGEING, _abi.LAW_SLIP):
            raise ValueError(f"law is {_abi.LAW_AGEING} or {_abi.LAW_SLIP} (RSF_LAW_*), not {codes[0]}")
        if codes[1] not in _OBSERVABLE_NAMES:
            raise ValueError(f"observable is one of {sorted(_OBSERVABLE_NAMES)} (RSF_OBS_*), not {codes[1]}")
        normal = lambda q, obs, fd: self.law_fit_normal(codes[0], codes[1], q, obs, fd)
        run = lambda q, obs, *rest: self.law_fit_run(codes[0], codes[1], q, obs, *rest)
        return self._fit_drive(normal, run, q0, data, lo, hi, fd_rel_step, ftol, max_iter, iters_per_launch,
                               ready=lambda: (self._law_fit_fn("rsf_law_fit_normal"), self._law_fit_fn("rsf_law_fit_run")))

    # -- the exact posterior on a tensor quadrature grid (include/rsf_grid.h) ------------------------------
    @staticmethod
    def _grid_axes(x, w=None):
        """x (and w): one array (d = 1) or a sequence of d arrays → (d, n (d,) int32, the nodes' list, x and w concatenated)"""
        xs = [np.ascontiguousarray(x, dtype=np.float64)] if np.ndim(x[0]) == 0 else [np.ascontiguousarray(a, dtype=np.float64) for a in x]
        d = len(xs)
        if not 1 <= d <= _abi.GRID_MAX_PARAMS or any(a.ndim != 1 for a in xs):
            raise ValueError(f"a grid has 1 to {_abi.GRID_MAX_PARAMS} axes, each a 1-D array of nodes")
        ws = None
        if w is not None:
            ws = [np.ascontiguousarray(w, dtype=np.float64)] if np.ndim(w[0]) == 0 else [np.ascontiguousarray(a, dtype=np.float64) for a in w]
            if [a.shape for a in ws] != [a.shape for a in xs]:
                raise ValueError("every axis has as many weights as nodes")
        n = np.array([a.size for a in xs], dtype=np.int32)
        return d, n, xs, np.concatenate(xs), None if ws is None else np.concatenate(ws)

    @staticmethod
    def _grid_coords(coords, d):
        c = _abi.GRID_COORDS.get(coords, coords) if isinstance(coords, str) else (_abi.GRID_PLAIN if coords is None else coords)
        if c not in (_abi.GRID_PLAIN, _abi.GRID_PRODUCT) or (c == _abi.GRID_PRODUCT and d != 3):
            raise ValueError("coords is 'plain' or, with three axes, 'product'")
        return int(c)

    def grid_logtarget(self, x, data, lo, hi, coords=None, shape=None):
        """rsf_grid_logtarget, the fused hot path: one float64 RK4 solve per node of the tensor grid with the axes x (d = 1 or 3),
        the node formed on the device from its flat index i0 + n0 (i1 + n1 i2) → (l (N,), ssq (N,)) in this engine's memory space.
        l = -shape log SSq (- log x1 with coords='product', where x0 = Dc a); -inf outside the CLOSED box [lo, hi] and where SSq is
        not finite.  shape defaults to nout / 2."""
        self._need_model()
        d, n, _, xc, _ = self._grid_axes(x)
        c = self._grid_coords(coords, d)
        obs = self._in(data)
        if obs.ndim != 1 or int(obs.shape[0]) != self.nout:
            raise ValueError(f"data has shape {tuple(obs.shape)}, the model produces {self.nout} samples")
        lo, hi = _vec(lo, d, "lo"), _vec(hi, d, "hi")
        N = int(np.prod(n.astype(np.int64)))
        l, ssq = self._empty((N,)), self._empty((N,))
        _abi.check(self.lib, self.lib.rsf_grid_logtarget(self._ctx, d, _i32p(n), _dp(xc), self._ptr(obs), float(0.5 * self.nout if shape is None else shape),
                                                         _dp(lo), _dp(hi), c, self._ptr(l), self._ptr(ssq)))
        return l, ssq

    def grid_columns(self, x, w, l, ssq, center=None, m0=True, cum0=True):
        """rsf_grid_columns: the fixed-order reductions of any l, ssq (N,) on the grid (x, w) → dict(lmax, center, fields
        (ncol, len(GRID_FIELDS)) and m0 (n0,) on the host, cum0 (ncol, n0) in this engine's memory space).  center: by default
        the middle node of axis 0."""
        d, n, xs, xc, wc = self._grid_axes(x, w)
        N, n0 = int(np.prod(n.astype(np.int64))), int(n[0])
        l, ssq = self._in(l), self._in(ssq)
        if math.prod(l.shape) != N or math.prod(ssq.shape) != N:
            raise ValueError(f"l and ssq hold one value per node: {N}")
        center = float(xs[0][n0 // 2]) if center is None else float(center)
        fields, vm0, vc0 = self._empty((N // n0, len(_abi.GRID_FIELDS))), self._empty((n0,)) if m0 else None, self._empty((N // n0, n0)) if cum0 else None
        lmax = ctypes.c_double()
        _abi.check(self.lib, self.lib.rsf_grid_columns(self._ctx, d, _i32p(n), _dp(xc), _dp(wc), self._ptr(l), self._ptr(ssq), center, ctypes.byref(lmax),
                                                       self._ptr(fields), self._ptr(vm0), self._ptr(vc0)))
        return {"lmax": lmax.value, "center": center, "fields": _host(fields), "m0": None if vm0 is None else _host(vm0), "cum0": vc0}

    def grid_finish(self, x, w, lo, hi, shape, lmax, fields, center, coords=None):
        """rsf_grid_finish (host only): the column fields taken at (center, lmax) → dict(Z, log_integral, log_evidence, n_neginf,
        mean (d,), cov (d, d), x0_mean, x0_var, std2_mean, std2_var, mass1 (n1,), mass2 (n2,), pair (n2, n1), cum1 (n2, n1),
        cum2 (n2,)).  A grid without a finite node: log_integral -inf, the rest NaN."""
        d, n, _, xc, wc = self._grid_axes(x, w)
        c = self._grid_coords(coords, d)
        n1, n2 = (int(n[1]) if d > 1 else 1), (int(n[2]) if d > 2 else 1)
        f = _host(fields).reshape(-1)
        if f.size != n1 * n2 * len(_abi.GRID_FIELDS):
            raise ValueError(f"fields is ({n1 * n2}, {len(_abi.GRID_FIELDS)})")
        lo, hi = _vec(lo, d, "lo"), _vec(hi, d, "hi")
        head, mass1, mass2 = np.empty(_abi.GRID_HEAD), np.empty(n1), np.empty(n2)
        pair, cum1, cum2 = np.empty((n2, n1)), np.empty((n2, n1)), np.empty(n2)
        _abi.check(self.lib, self.lib.rsf_grid_finish(d, _i32p(n), _dp(xc), _dp(wc), c, float(center), float(shape), _dp(lo), _dp(hi), float(lmax), _dp(f),
                                                      _dp(head), _dp(mass1), _dp(mass2), _dp(pair), _dp(cum1), _dp(cum2)))
        out = {k: float(head[i]) for k, i in _abi.GRID_HEAD_SCALARS.items()}
        out["n_neginf"] = int(head[3])
        out.update(mean=head[4:4 + d].copy(), cov=head[7:16].reshape(3, 3)[:d, :d].copy(), mass1=mass1, mass2=mass2, pair=pair, cum1=cum1, cum2=cum2)
        return out

    def grid_draw(self, x, cum0, cum1, cum2, n, coords=None, seed=0, offset=0, cells=False):
        """rsf_grid_draw: n independent draws by inverting the cumulative tables with the uniforms of smc_init's stream
        (seed, offset + j) → q (n, d) in this engine's memory space; with cells=True also the cell of each axis, (n, d) int32 on
        the host."""
        d, nn, _, xc, _ = self._grid_axes(x)
        c = self._grid_coords(coords, d)
        n = int(n)
        cum0 = self._in(cum0)
        if math.prod(cum0.shape) != int(np.prod(nn.astype(np.int64))):
            raise ValueError("cum0 holds one value per node")
        c1 = _host(cum1).reshape(-1) if d > 1 else None
        c2 = _host(cum2).reshape(-1) if d > 2 else None
        if (d > 1 and c1.size != int(nn[1]) * (int(nn[2]) if d > 2 else 1)) or (d > 2 and c2.size != int(nn[2])):
            raise ValueError("cum1 is (n2, n1) and cum2 (n2,)")
        q = self._empty((max(n, 0), d))
        cell = None
        if cells:
            cell = self._torch.empty((max(n, 0), d), dtype=self._torch.int32, device=f"cuda:{self.device}") if self.mem == "device" else np.empty((max(n, 0), d), dtype=np.int32)
        _abi.check(self.lib, self.lib.rsf_grid_draw(self._ctx, d, _i32p(nn), _dp(xc), c, self._ptr(cum0), None if c1 is None else _dp(c1),
                                                    None if c2 is None else _dp(c2), int(seed), int(offset), n, self._ptr(q), self._ptr(cell)))
        return (q, np.asarray(cell.cpu() if hasattr(cell, "cpu") else cell)) if cells else q

    def grid_cdf(self, x, cum0, pair, xs, coords=None):
        """rsf_grid_cdf: the CDF of q0 (Dc, also where the grid's axis is Dc a) at the points xs → (len(xs),) on the host."""
        d, nn, _, xc, _ = self._grid_axes(x)
        c = self._grid_coords(coords, d)
        cum0, pr = self._in(cum0), _host(pair).reshape(-1)
        xs = np.ascontiguousarray(np.atleast_1d(np.asarray(xs, dtype=np.float64)))
        if math.prod(cum0.shape) != int(np.prod(nn.astype(np.int64))) or pr.size * int(nn[0]) != math.prod(cum0.shape) or xs.ndim != 1:
            raise ValueError("cum0 holds one value per node, pair one per column, xs is 1-D")
        F = np.empty(xs.size)
        _abi.check(self.lib, self.lib.rsf_grid_cdf(self._ctx, d, _i32p(nn), _dp(xc), c, self._ptr(cum0), _dp(pr), int(xs.size), _dp(xs), _dp(F)))
        return F

    def _grid_result(self, x, w, l, ssq, lo, hi, shape, coords, ltarget, outside=0.0, n_solves=0):
        d, n, xs, _, wc = self._grid_axes(x, w)
        ws = np.split(wc, np.cumsum(n)[:-1])
        c = self._grid_coords(coords, d)
        col = self.grid_columns(xs, ws, l, ssq)
        fin = self.grid_finish(xs, ws, lo, hi, shape, col["lmax"], col["fields"], col["center"], c)
        return GridPosterior(self, xs, ws, c, _vec(lo, d, "lo"), _vec(hi, d, "hi"), float(shape), col, fin, ltarget, float(outside), int(n_solves))

    def grid_from_ssq(self, ssq_fn, x, w, lo, hi, shape, coords=None, outside=0.0):
        """The grid posterior with the caller's sum of squares (the duck-typed model contract, the closed forms): ssq_fn(points
        (m, d) float64 on the host, natural coordinates q) → SSq (m,), called for the nodes inside the closed box.  d = 1..3, no
        model needed; the reductions, the tables, the draws and the CDF are the GPU's.  → GridPosterior."""
        d, n, xs, _, _ = self._grid_axes(x, w)
        c = self._grid_coords(coords, d)
        lo, hi, shape = _vec(lo, d, "lo"), _vec(hi, d, "hi"), float(shape)
        q = np.stack([np.ravel(a, order="F") for a in np.meshgrid(*xs, indexing="ij")], axis=1)
        jac = 0.0
        if c == _abi.GRID_PRODUCT:
            jac = -np.log(q[:, 1])
            q[:, 0] = q[:, 0] / q[:, 1]

        def ltarget(pts, jac=0.0):
            pts = np.asarray(pts, dtype=np.float64).reshape(-1, d)
            inb = ((pts >= lo) & (pts <= hi)).all(axis=1)
            s = np.full(pts.shape[0], np.nan)
            if inb.any():
                s[inb] = np.asarray(ssq_fn(pts[inb]), dtype=np.float64).reshape(-1)
            ok = inb & np.isfinite(s) & (s > 0)
            with np.errstate(divide="ignore", invalid="ignore"):
                return np.where(ok, -shape * np.log(np.where(ok, s, 1.0)) + jac, -np.inf), s

        l, ssq = ltarget(q, jac)
        return self._grid_result(xs, w, l, ssq, lo, hi, shape, c, lambda pts: self._in(ltarget(_host(pts))[0]), outside, int(np.isfinite(ssq).sum()))

    def grid_posterior(self, data, lo, hi, n=None, coords=None, window_sd=12.0, shape=None, n_coarse=None, ssq_fn=None):
        """The exact posterior of the device model (set_model) given `data` over the closed box [lo, hi], d = 1 (Dc) or 3 (Dc, a, b),
        by quadrature on the GPU in two stages (the procedure of the test-suite's reference quadrature).  A coarse scan of the whole
        box — d = 1: n_coarse (4001) linearly and as many logarithmically spaced nodes strictly inside, trapezoid weights; d = 3: a
        coarse axis (801 + 801) in Dc a at the first, middle and last (a, b) nodes — finds the mass: the window is mean +- window_sd
        SD (of the widest column at d = 3), clipped to the box, and `outside` the coarse mass beyond it.  The fine grid: d = 1,
        n = (4001,) Simpson nodes on the window; d = 3, n = (2001, 65, 65): coords 'product' (axis 0 is Dc a, which straightens the
        ridge Dc a = const), axes 1 and 2 uniform over [lo, hi] with the faces, Simpson on every axis (odd n).  → GridPosterior.
        ssq_fn (d = 1 only; data is then not read): the same two stages with the nodes' sums of squares from the caller — ssq_fn(points
        (m, 1) float64 on the host) → SSq (m,), as grid_from_ssq calls it; law_ssq_fn(law, data) makes one for either state law."""
        self._need_model(law_aware=ssq_fn is not None, stiff_aware=ssq_fn is not None)
        blo, bhi, d = self._smc_box(lo, hi)
        if d not in (1, 3):
            raise ValueError("the box has d = 1 (Dc) or 3 (Dc, a, b) parameters")
        if ssq_fn is not None and d != 1:
            raise NotImplementedError("grid_posterior takes an ssq_fn at d = 1 only (d = 3: grid_from_ssq on the caller's grid)")
        shape = 0.5 * self.nout if shape is None else float(shape)
        n = ((4001,) if d == 1 else (2001, 65, 65)) if n is None else tuple(int(v) for v in np.atleast_1d(n))
        if len(n) != d or any(v < 3 or v % 2 == 0 for v in n):
            raise ValueError(f"n holds {d} odd node counts >= 3 (composite Simpson)")
        c = self._grid_coords(("product" if d == 3 else "plain") if coords is None else coords, d)
        if ssq_fn is None:
            obs = self._in(data)
            ltarget = lambda pts: self.evidence_logtarget(pts, obs, blo, bhi, self._in(np.zeros(int(math.prod(pts.shape)) // d)), shape)
            nodes = lambda x: self.grid_logtarget(x, obs, blo, bhi, c, shape)
        else:
            def host_target(pts):  # grid_from_ssq's: -inf outside the closed box and where SSq is not finite and > 0
                pts = np.asarray(pts, dtype=np.float64).reshape(-1, 1)
                inb = ((pts >= blo) & (pts <= bhi)).all(axis=1)
                s = np.full(pts.shape[0], np.nan)
                if inb.any():
                    s[inb] = np.asarray(ssq_fn(pts[inb]), dtype=np.float64).reshape(-1)
                ok = inb & np.isfinite(s) & (s > 0)
                return np.where(ok, -shape * np.log(np.where(ok, s, 1.0)), -np.inf), s

            ltarget = lambda pts: self._in(host_target(_host(pts))[0])
            nodes = lambda x: tuple(self._in(v) for v in host_target(x[0]))
        nc = (4001 if d == 1 else 801) if n_coarse is None else int(n_coarse)
        prod = c == _abi.GRID_PRODUCT
        alo, ahi = (blo[0] * blo[1], bhi[0] * bhi[1]) if prod else (blo[0], bhi[0])  # the range of axis 0
        xc = np.linspace(alo, ahi, nc)
        if alo >= 0:
            xc = np.union1d(xc, np.geomspace(max(alo, 1e-6 * ahi), ahi, nc))
        xc = xc[(xc > alo) & (xc < ahi)]
        wc = np.zeros_like(xc)
        wc[:-1] += 0.5 * np.diff(xc)
        wc[1:] += 0.5 * np.diff(xc)
        fine = [_simpson_axis(blo[p], bhi[p], n[p]) for p in range(1, d)]
        sel = [a[0][[0, a[0].size // 2, a[0].size - 1]] for a in fine]
        cx, cw = [xc] + sel, [wc] + [np.ones(3)] * (d - 1)
        l, ssq = nodes(cx)
        col = self.grid_columns(cx, cw, l, ssq, m0=False, cum0=False)
        f = col["fields"]
        if not (f[:, 0] > 0).any():
            raise _abi.RsfError(-1, "Engine.grid_posterior: the target has no mass inside the box")
        ok = f[:, 0] > 0
        mc = col["center"] + f[ok, 1] / f[ok, 0]
        sc = np.sqrt(np.maximum(f[ok, 2] / f[ok, 0] - (f[ok, 1] / f[ok, 0]) ** 2, 0.0))
        wlo, whi = max(float((mc - window_sd * sc).min()), alo), min(float((mc + window_sd * sc).max()), ahi)
        if not wlo < whi:
            raise _abi.RsfError(-1, "Engine.grid_posterior: the coarse scan does not resolve the posterior (no spread on the coarse axis)")
        e = np.exp(np.where(np.isfinite(_host(l)), _host(l) - col["lmax"], -np.inf)).reshape(-1, xc.size)
        out = (xc < wlo) | (xc > whi)
        outside = float(((wc * e)[:, out].sum(axis=1)[ok] / f[ok, 0]).max()) if out.any() else 0.0
        x0 = _simpson_axis(wlo, whi, n[0])
        xs, ws = [x0[0]] + [a[0] for a in fine], [x0[1]] + [a[1] for a in fine]
        l, ssq = nodes(xs)
        return self._grid_result(xs, ws, l, ssq, blo, bhi, shape, c, ltarget, outside, int(xc.size * 3 ** (d - 1) + math.prod(n)))

    # -- the exact posterior of a state-law model on a grid in the coordinates of a fit (include/rsf_law_grid.h) ----------
    def _law_grid_fn(self, name):
        """a function of include/rsf_law_grid.h, which librsf_hip.so alone exports"""
        try:
            return getattr(self.lib, name)
        except AttributeError:
            raise _abi.RsfError(-5, f"{name} is exported by librsf_hip.so only: the {self.lib.rsf_backend().decode()!r} library has no such "
                                    "symbol (include/rsf_law_grid.h)") from None

    @staticmethod
    def _law_grid_map(d, m, L, tr, perm):
        """the map (m (d,), L (d, d) lower-triangular, tr, perm) as the library takes it → (m, packed L, tr int32, perm int32)"""
        m = np.ascontiguousarray(np.asarray(m, dtype=np.float64).reshape(-1))
        L = np.asarray(L, dtype=np.float64)
        if m.shape != (d,) or L.shape != (d, d):
            raise ValueError(f"the map is m ({d},) and a lower-triangular L ({d}, {d})")
        if np.any(np.triu(L, 1) != 0.0):
            raise ValueError("L is lower-triangular: an entry above its diagonal is not 0")
        tr = np.zeros(d, dtype=np.int32) if tr is None else np.ascontiguousarray(np.asarray(tr).reshape(-1) != 0, dtype=np.int32)
        perm = np.arange(d, dtype=np.int32) if perm is None else np.ascontiguousarray(np.asarray(perm).reshape(-1), dtype=np.int32)
        if tr.shape != (d,) or perm.shape != (d,) or sorted(perm.tolist()) != list(range(d)):
            raise ValueError(f"tr holds {d} flags and perm is a permutation of 0 .. {d - 1}")
        return m, np.ascontiguousarray(L[np.tril_indices(d)]), tr, perm

    def law_logtarget(self, law, observable, data, lo, hi, z=None, m=None, L=None, tr=None, perm=None, theta=None, logg=None, shape=None,
                      want_q=False):
        """rsf_law_logtarget, the fused hot path: one float64 RK4 solve under `law` per point with the running sum of squares of
        `observable` against data → (l (N,), ssq (N,)[, q (N, d)]) in this engine's memory space.  The points are the nodes of the
        grid with the axes z (d = 1 or 3) under the map phi = m + L z, q_perm[p] = phi_p or exp(phi_p) where tr[p] — or, with
        theta (N,) / (N, d) given, those points in the order (Dc, a, b), with logg (N,) subtracted (tr and perm then say which
        parameters' logarithms enter: evidence_logtarget's Jacobian).  l = -shape log SSq + J - logg, -inf outside the CLOSED box
        [lo, hi] and where SSq is not finite; ssq is NaN outside the box.  want_q: also the point every lane solved.  shape
        defaults to nout / 2."""
        self._need_model(law_aware=True)
        lw, ob = self._law_codes(law, observable)
        obs = self._in(data)
        if obs.ndim != 1 or int(obs.shape[0]) != self.nout:
            raise ValueError(f"data has shape {tuple(obs.shape)}, the model produces {self.nout} samples")
        if (theta is None) == (z is None):
            raise ValueError("the points are either the nodes of the axes z or theta, not both and not neither")
        if theta is None:
            d, n, _, zc, _ = self._grid_axes(z)
            if m is None or L is None:
                raise ValueError("a grid needs the map: m and L")
            N, x, g, npts = int(np.prod(n.astype(np.int64))), None, None, 0
            if logg is not None:
                raise ValueError("logg goes with theta")
        else:
            x = self._in(theta)
            if x.ndim == 1:
                x = x.reshape(-1, 1)
            N, d = int(x.shape[0]), int(x.shape[1])
            n = zc = None
            npts = N
            g = None if logg is None else self._in(logg)
            if g is not None and math.prod(g.shape) != N:
                raise ValueError(f"logg holds {math.prod(g.shape)} values, theta {N} points")
        if d not in (1, 3):
            raise ValueError("the points have d = 1 (Dc) or 3 (Dc, a, b) parameters")
        if theta is None:
            mm, Lp, tr, perm = self._law_grid_map(d, m, L, tr, perm)
        else:
            mm, Lp, tr, perm = self._law_grid_map(d, np.zeros(d), np.eye(d), tr, perm)
        lo, hi = _vec(lo, d, "lo"), _vec(hi, d, "hi")
        l, ssq, qo = self._empty((N,)), self._empty((N,)), self._empty((N, d)) if want_q else None
        _abi.check(self.lib, self._law_grid_fn("rsf_law_logtarget")(
            self._ctx, lw, ob, d, None if n is None else _i32p(n), None if zc is None else _dp(zc), _dp(mm), _dp(Lp), _i32p(tr), _i32p(perm), npts,
            self._ptr(x), self._ptr(g), self._ptr(obs), float(0.5 * self.nout if shape is None else shape), _dp(lo), _dp(hi), self._ptr(l),
            self._ptr(ssq), self._ptr(qo)))
        return (l, ssq, qo) if want_q else (l, ssq)

    def law_grid_moments(self, z, w, m, L, tr, perm, l, ssq, lmax, center, return_fields=False):
        """rsf_law_grid_moments: the fixed-order sums over the grid of W e times {1, dq_p, dq_p dq_r, SSq, SSq^2} in natural
        coordinates, dq = q - center (center in the order (Dc, a, b)), e = exp(l - lmax) → the totals (len(LAW_GRID_FIELDS),) on the
        host; return_fields: also the per-column sums (ncol, len(LAW_GRID_FIELDS)) the totals were added from, in index order."""
        d, n, _, zc, wc = self._grid_axes(z, w)
        if d not in (1, 3):
            raise ValueError("the grid has d = 1 or 3 axes")
        mm, Lp, tr, perm = self._law_grid_map(d, m, L, tr, perm)
        N = int(np.prod(n.astype(np.int64)))
        l, ssq = self._in(l), self._in(ssq)
        if math.prod(l.shape) != N or math.prod(ssq.shape) != N:
            raise ValueError(f"l and ssq hold one value per node: {N}")
        c = _vec(center, d, "center")
        nf = len(_abi.LAW_GRID_FIELDS)
        fields, total = self._empty((N // int(n[0]), nf)) if return_fields else None, np.empty(nf)
        _abi.check(self.lib, self._law_grid_fn("rsf_law_grid_moments")(self._ctx, d, _i32p(n), _dp(zc), _dp(wc), _dp(mm), _dp(Lp), _i32p(tr), _i32p(perm),
                                                                       self._ptr(l), self._ptr(ssq), float(lmax), _dp(c), self._ptr(fields), _dp(total)))
        return (total, _host(fields)) if return_fields else total

    def law_grid_posterior(self, law, observable, data, lo, hi, center, factor, log_coords=None, first=0, n=None, window_sd=8.0, shape=None,
                           edge_tol=1e-8):
        """The exact posterior of the device model (set_model) under the state law `law` given `data`, a series of `observable`, over
        the closed box [lo, hi], d = 1 (Dc) or 3 (Dc, a, b), by quadrature on a tensor grid laid in the coordinates of a fit.
        center (d,): the fit's point; factor (d, d): a factor F of the fit's covariance F F^T in the working coordinates
        phi_p = q_p, or log q_p for the parameters log_coords names ("Dc", "a", "b" or their indices; the covariance of log q_p is
        that of q_p divided by q_p^2).  first: the parameter on axis 0 (the covariance is permuted and factored again, so that L
        is lower-triangular with `first` in front): marginal, quantiles and cdf are that parameter's.  Simpson axes of odd n[p]
        nodes on [-window_sd, window_sd] per z-axis, by default 65 each.  An axis whose two end nodes carry more than edge_tol of
        its marginal mass has its window doubled at the same node spacing, at most twice; then RsfError names the axis.
        → LawGridPosterior."""
        self._need_model(law_aware=True)
        blo, bhi, d = self._smc_box(lo, hi)
        if d not in (1, 3):
            raise ValueError("the box has d = 1 (Dc) or 3 (Dc, a, b) parameters")
        names = ("Dc", "a", "b")[:d]
        idx = lambda v: names.index(v) if isinstance(v, str) and v in names else int(v)
        try:
            first = idx(first)
            logged = sorted({idx(v) for v in (log_coords or ())})
        except (TypeError, ValueError):
            raise ValueError(f"first and log_coords name parameters of {names} (or their indices)") from None
        if not 0 <= first < d or any(not 0 <= p < d for p in logged):
            raise ValueError(f"first and log_coords name parameters of {names} (or their indices)")
        q0 = _vec(center, d, "center")
        F = np.asarray(factor, dtype=np.float64)
        if F.shape != (d, d) or not np.isfinite(F).all():
            raise ValueError(f"factor is a finite ({d}, {d}) factor of the fit's covariance")
        if np.any((q0 < blo) | (q0 > bhi)):
            raise ValueError("center lies outside the box")
        if any(not blo[p] > 0 for p in logged):
            raise ValueError("a logged parameter needs lo > 0")
        n = (65,) * d if n is None else tuple(int(v) for v in np.atleast_1d(n))
        if len(n) != d or any(v < 3 or v % 2 == 0 for v in n):
            raise ValueError(f"n holds {d} odd node counts >= 3 (composite Simpson)")
        if not float(window_sd) > 0:
            raise ValueError("window_sd must be > 0")
        shape = 0.5 * self.nout if shape is None else float(shape)
        perm = np.array([first] + [p for p in range(d) if p != first], dtype=np.int32)
        tr = np.array([1 if p in logged else 0 for p in perm], dtype=np.int32)
        m = np.where(tr == 1, np.log(np.where(tr == 1, q0[perm], 1.0)), q0[perm])
        try:
            L = np.linalg.cholesky((F @ F.T)[np.ix_(perm, perm)])
        except np.linalg.LinAlgError:
            raise _abi.RsfError(_abi.ERR_NOT_POSDEF, "Engine.law_grid_posterior: factor factor^T is not positive definite") from None
        obs = self._in(data)
        n, win, solves = list(n), [float(window_sd)] * d, 0
        for attempt in range(3):
            zw = [_simpson_axis(-win[p], win[p], n[p]) for p in range(d)]
            z, w = [a[0] for a in zw], [a[1] for a in zw]
            l, ssq = self.law_logtarget(law, observable, obs, blo, bhi, z=z, m=m, L=L, tr=tr, perm=perm, shape=shape)
            solves += math.prod(n)
            col = self.grid_columns(z, w, l, ssq, center=0.0)
            if not np.isfinite(col["lmax"]):
                raise _abi.RsfError(-1, "Engine.law_grid_posterior: the target has no mass on the grid (every node is outside the box or has no finite SSq)")
            fin = self.grid_finish(z, w, blo, bhi, shape, col["lmax"], col["fields"], 0.0, _abi.GRID_PLAIN)
            centre = np.where(tr == 1, np.exp(m), m)
            cq = np.empty(d)
            cq[perm] = centre
            mom = self.law_grid_moments(z, w, m, L, tr, perm, l, ssq, col["lmax"], cq)
            res = LawGridPosterior(self, law, observable, obs, z, w, (m, L, tr, perm), blo, bhi, shape, l, ssq, col, fin, mom, cq, solves, win)
            bad = np.flatnonzero(res.edge_masses > float(edge_tol))
            if bad.size == 0:
                return res
            if attempt == 2:
                p = int(bad[np.argmax(res.edge_masses[bad])])
                raise _abi.RsfError(-1, f"Engine.law_grid_posterior: axis {p} (parameter {names[int(perm[p])]!r} in front) still carries "
                                        f"{res.edge_masses[p]:.3e} of its mass on its end nodes at a window of {win[p]:g} SD: the fit's "
                                        "covariance does not describe the posterior")
            for p in bad:
                n[p], win[p] = 2 * n[p] - 1, 2.0 * win[p]

    def law_evidence(self, law, observable, samples, data, lo, hi, shape=None, transform=None, n_proposal=None, fit_fraction=0.5, seed=0,
                     ess_factor=None):
        """evidence — its arguments, its driver and its result — for the device model under the state law `law` and a series `data`
        of `observable`: the target of every draw is law_logtarget's on points, one fused solve per draw."""
        self._need_model(law_aware=True)
        shape = 0.5 * self.nout if shape is None else float(shape)
        obs = self._in(data)
        d = int(np.shape(samples)[-1]) if np.ndim(samples) > 1 else 1
        tr = self._ev_flags(transform, d)
        return self._evidence(samples, lambda theta, logg: self.law_logtarget(law, observable, obs, lo, hi, theta=theta, logg=logg, tr=tr, shape=shape)[0],
                              lo, hi, shape, self.nout, transform, n_proposal, fit_fraction, seed, ess_factor)

    # -- convergence diagnostics of a kept trace (include/rsf_diag.h) --------------------------
    def _diag_trace(self, trace):
        x = self._in(trace)
        if x.ndim == 2:
            x = x.reshape(int(x.shape[0]), int(x.shape[1]), 1)
        if x.ndim != 3:
            raise ValueError("a trace is (n_iters, n_chains) or (n_iters, n_chains, n_params)")
        return x, int(x.shape[0]), int(x.shape[1]), int(x.shape[2])

    @staticmethod
    def _diag_center(x, d, center):
        if center is None:  # the trace's first draw of chain 0
            return _host(x[0, 0]).reshape(d)
        return _vec(center, d, "center")

    def diag_partials(self, trace, superchain_size=None, center=None, lag_begin=0, lag_end=None):
        """rsf_diag_partials: the additive partials of the trace (n, C[, d]) about `center` (default: the first draw of chain 0)
        for the lags [lag_begin, lag_end) (default: every lag, N = n // 2) → (d, DIAG_HEAD + L) float64 on the host.  Partials of
        disjoint sets of chains taken about the same centre add (dist.allreduce_diag_partials); a superchain must not straddle
        two sets."""
        x, n, C, d = self._diag_trace(trace)
        c = self._diag_center(x, d, center)
        lag_end = n // 2 if lag_end is None else int(lag_end)
        out = np.empty((d, _abi.DIAG_HEAD + max(lag_end - int(lag_begin), 0)))
        _abi.check(self.lib, self.lib.rsf_diag_partials(self._ctx, n, C, d, self._ptr(x), int(superchain_size or 0), _dp(c),
                                                        int(lag_begin), lag_end, _dp(out)))
        return out

    def diag_finish(self, n_iters, partials, center, superchain_size=None, n_lags=None):
        """rsf_diag_finish (host only): the statistics of summed partials whose lags are [0, n_lags) → one dict per parameter
        (split_rhat, nested_rhat, ess, tau, mcse_mean, mean, var_plus, W, B_over_N, K, lags_complete)."""
        part = _host(partials)
        part = part.reshape(-1, part.shape[-1])
        d = int(part.shape[0])
        n_lags = int(part.shape[1]) - _abi.DIAG_HEAD if n_lags is None else int(n_lags)
        if part.shape[1] != _abi.DIAG_HEAD + n_lags:
            raise ValueError(f"partials have {part.shape[1] - _abi.DIAG_HEAD} lags, not n_lags = {n_lags}")
        c = _vec(center, d, "center")
        out = np.empty((d, len(_abi.DIAG_OUT)))
        _abi.check(self.lib, self.lib.rsf_diag_finish(int(n_iters), d, int(superchain_size or 0), _dp(c),
                                                      _dp(part), n_lags, _dp(out)))
        res = []
        for row in out:
            r = dict(zip(_abi.DIAG_OUT, (float(v) for v in row)))
            r["K"], r["lags_complete"], r["n_lags"] = int(r["K"]), bool(r["lags_complete"]), n_lags
            res.append(r)
        return res

    def diagnostics(self, trace, superchain_size=None, center=None, n_lags=None, lag_block=64):
        """Split R-hat, nested R-hat (superchains of `superchain_size` consecutive chains) and the multi-chain ESS of a trace
        (n, C[, d]) → one dict per parameter (see diag_finish; `n_lags` = the lags used).  Without `n_lags` the lags are computed
        `lag_block` at a time until Geyer's truncation is reached for every parameter; with it, exactly [0, n_lags) and
        `lags_complete` says whether that was enough."""
        x, n, _, d = self._diag_trace(trace)
        c = self._diag_center(x, d, center)
        if n_lags is not None:
            return self.diag_finish(n, self.diag_partials(x, superchain_size, c, 0, n_lags), c, superchain_size)
        if int(lag_block) < 2:
            raise ValueError("lag_block must be >= 2")
        return _lag_blocks(n // 2, lag_block, lambda b, e: self.diag_partials(x, superchain_size, c, b, e),
                           lambda part: self.diag_finish(n, part, c, superchain_size), lambda res: all(r["lags_complete"] for r in res))[1]

    # -- rank-normalised diagnostics and order statistics (include/rsf_diag.h, rsf_diag_rank_*) -----------
    def rank_prepare(self, trace, probs=(), hdi_prob=0.94, series=False):
        """rsf_diag_rank_prepare: sort every parameter's draws on the device and keep the four derived series (zb, zf, I_lo, I_hi) in
        this engine's rank workspace → stats (d, len(DIAG_RANK_STATS) + len(probs)) on the host, and with series=True also a copy of
        the series (4, n, C, d) in this engine's memory space.  rank_partials then reads the workspace; rank_release frees it."""
        x, n, C, d = self._diag_trace(trace)
        pr = np.ascontiguousarray(np.asarray(probs, dtype=np.float64).reshape(-1))
        stats = np.empty((d, len(_abi.DIAG_RANK_STATS) + pr.size))
        out = self._empty((4, n, C, d)) if series else None
        _abi.check(self.lib, self.lib.rsf_diag_rank_prepare(self._ctx, n, C, d, self._ptr(x), int(pr.size), _dp(pr),
                                                            float(hdi_prob), _dp(stats), self._ptr(out)))
        self._rank_d = d
        return (stats, out) if series else stats

    def rank_partials(self, lag_begin, lag_end):
        """rsf_diag_rank_partials: the diagnostics partials of the four prepared series → (4, d, DIAG_HEAD + L) on the host."""
        d = getattr(self, "_rank_d", None)
        if d is None:
            raise ValueError("rank_partials before rank_prepare")
        out = np.empty((4, d, _abi.DIAG_HEAD + max(int(lag_end) - int(lag_begin), 0)))
        _abi.check(self.lib, self.lib.rsf_diag_rank_partials(self._ctx, int(lag_begin), int(lag_end),
                                                             _dp(out)))
        return out

    def rank_finish(self, n_iters, stats, partials, n_lags=None):
        """rsf_diag_rank_finish (host only) → (d, len(DIAG_RANK_OUT)) float64."""
        st = np.ascontiguousarray(np.asarray(stats, dtype=np.float64))
        part = np.ascontiguousarray(np.asarray(partials, dtype=np.float64))
        d = int(st.shape[0])
        n_lags = int(part.shape[-1]) - _abi.DIAG_HEAD if n_lags is None else int(n_lags)
        if part.shape != (4, d, _abi.DIAG_HEAD + n_lags):
            raise ValueError(f"partials must be (4, {d}, DIAG_HEAD + n_lags), not {part.shape}")
        out = np.empty((d, len(_abi.DIAG_RANK_OUT)))
        _abi.check(self.lib, self.lib.rsf_diag_rank_finish(int(n_iters), d, _dp(st), int(st.shape[1]) - len(_abi.DIAG_RANK_STATS),
                                                           _dp(part), n_lags, _dp(out)))
        return out

    def rank_release(self):
        self._rank_d = None
        _abi.check(self.lib, self.lib.rsf_diag_rank_release(self._ctx))

    def rank_diagnostics(self, trace, probs=(0.025, 0.5, 0.975), hdi_prob=0.94, n_lags=None, lag_block=64):
        """Rank-normalised R-hat (max of bulk and folded-tail split R-hat), bulk and tail ESS, median, quantiles and the HDI of a
        trace (n, C[, d]), as ArviZ reports them (include/rsf_diag.h) → one dict per parameter: rhat, rhat_bulk, rhat_tail,
        ess_bulk, ess_tail, ess_q05, ess_q95, median, quantiles {prob: value}, hdi (lo, hi), n_lags, lags_complete.  The trace
        is sorted once; the lags of the four derived series are then computed `lag_block` at a time until Geyer's truncation is
        reached for all of them (or exactly [0, n_lags)).  The rank workspace is freed before returning."""
        x, n, _, d = self._diag_trace(trace)
        probs = tuple(float(p) for p in probs)
        if n_lags is None and int(lag_block) < 2:
            raise ValueError("lag_block must be >= 2")
        stats = self.rank_prepare(x, probs, hdi_prob)
        try:
            if n_lags is not None:
                part = self.rank_partials(0, int(n_lags))
                out = self.rank_finish(n, stats, part)
            else:
                part, out = _lag_blocks(n // 2, lag_block, self.rank_partials, lambda part: self.rank_finish(n, stats, part),
                                        lambda out: np.all(out[:, -1] != 0))
        finally:
            self.rank_release()
        L = part.shape[-1] - _abi.DIAG_HEAD
        res = []
        for p in range(d):
            r = dict(zip(_abi.DIAG_RANK_OUT, (float(v) for v in out[p])))
            st = dict(zip(_abi.DIAG_RANK_STATS, (float(v) for v in stats[p])))
            r["lags_complete"], r["n_lags"] = bool(r["lags_complete"]), L
            r["median"] = st["median"]
            r["quantiles"] = {pr: float(v) for pr, v in zip(probs, stats[p, len(_abi.DIAG_RANK_STATS):])}
            r["hdi"] = (st["hdi_lo"], st["hdi_hi"])
            res.append(r)
        return res

    # -- posterior predictive checks of pooled draws (include/rsf_predict.h) ---------------------
    def _predict_args(self, q, std2, data, law_aware=False, stiff_aware=False):
        self._need_model(law_aware, stiff_aware)
        q, std2, data = self._in(q), self._in(std2), self._in(data)
        if q.ndim == 1:
            q = q.reshape(-1, 1)
        if q.ndim != 2 or int(q.shape[1]) not in (1, 3):
            raise ValueError("draws are (n,) or (n, d) with d = 1 (Dc) or 3 (Dc, a, b)")
        n = int(q.shape[0])
        if n < 1:
            raise ValueError("no draws")
        if std2.ndim != 1 or int(std2.shape[0]) != n:
            raise ValueError(f"std2 has shape {tuple(std2.shape)}, the draws are {n}")
        if data.ndim != 1 or int(data.shape[0]) != self.nout:
            raise ValueError(f"data has shape {tuple(data.shape)}, the model produces {self.nout} samples")
        return q, std2, data, n, int(q.shape[1])

    def _predict_centers(self, center_y, center_l, rows=None):
        c = []
        for v in (center_y, center_l):
            v = _host(v)
            if rows is None and v.shape != (self.nout,):
                raise ValueError(f"a centre has shape {v.shape}, the model produces {self.nout} samples")
            if rows is not None and v.shape != (rows,):
                raise ValueError(f"a centre has shape {v.shape}, the series has {rows} rows")
            c.append(v)
        return c

    def predictive_partials(self, q, std2, data, center_y, center_l, return_series=False):
        """rsf_predict_partials: one forward solve per draw (q (n,) or (n, d), std2 (n,)) and the additive partials of the
        predictive statistics about the centres center_y, center_l (nout,) → (PREDICT_HEAD + nout * len(PREDICT_FIELDS),)
        float64 on the host; with return_series also the series (nout, n) in this engine's memory space.  Partials of disjoint
        shards of a pool taken about the same centres add (dist.allreduce_predictive_partials)."""
        return self._partials(lambda *a: self.lib.rsf_predict_partials(self._ctx, *a), False, q, std2, data, center_y, center_l, return_series)

    def _partials(self, call, law_aware, q, std2, data, center_y, center_l, return_series):
        """predictive_partials' and law_predictive_partials' body; call: the entry point behind its leading arguments"""
        q, std2, data, n, d = self._predict_args(q, std2, data, law_aware)
        cy, cl = self._predict_centers(center_y, center_l)
        series = None
        if return_series:
            try:
                series = self._empty((self.nout, n))
            except (MemoryError, RuntimeError) as e:
                raise MemoryError(f"cannot allocate the predictive series ({self.nout} x {n} doubles = {8 * self.nout * n} bytes); "
                                  "pass fewer draws (max_draws)") from e
        out = np.empty(_abi.PREDICT_HEAD + self.nout * len(_abi.PREDICT_FIELDS))
        try:
            _abi.check(self.lib, call(n, d, self._ptr(q), self._ptr(std2), self._ptr(data), _dp(cy), _dp(cl), _dp(out), self._ptr(series)))
        except _abi.RsfError as e:
            if e.code == -4:  # RSF_ERR_NOMEM
                raise _abi.RsfError(e.code, f"{e}; pass fewer draws (max_draws)") from e
            raise
        return (out, series) if return_series else out

    def predictive_finish(self, partials, center_y, center_l):
        """rsf_predict_finish (host only): the statistics of summed partials → dict of (nout,) arrays mean, var, pit, lpd,
        p_waic_k and the totals mean_std2, elpd_waic, p_waic, elpd_waic_se, n."""
        part = _host(partials).reshape(-1)
        nf = len(_abi.PREDICT_FIELDS)
        if part.size <= _abi.PREDICT_HEAD or (part.size - _abi.PREDICT_HEAD) % nf:
            raise ValueError(f"partials have {part.size} entries, not PREDICT_HEAD + rows * {nf}")
        rows = (part.size - _abi.PREDICT_HEAD) // nf
        cy = np.ascontiguousarray(np.asarray(center_y, dtype=np.float64))
        cl = np.ascontiguousarray(np.asarray(center_l, dtype=np.float64))
        if cy.shape != (rows,) or cl.shape != (rows,):
            raise ValueError(f"the centres have shapes {cy.shape}, {cl.shape}, the partials {rows} rows")
        out = np.empty((rows, len(_abi.PREDICT_OUT)))
        tot = np.empty(len(_abi.PREDICT_TOTALS))
        _abi.check(self.lib, self.lib.rsf_predict_finish(rows, _dp(part), _dp(cy), _dp(cl),
                                                         _dp(out), _dp(tot)))
        res = _rows_totals(out, tot, _abi.PREDICT_OUT, _abi.PREDICT_TOTALS)
        res["n"] = int(part[0])
        return res

    def predictive_quantiles(self, series, probs):
        """rsf_predict_quantiles: np.quantile(series, probs, axis=1) (method "linear", exact) of a series (nout, n) in this
        engine's memory space → (len(probs), nout) float64 on the host."""
        probs = _probs(probs, False, False, "probs")
        x = self._in(series)
        rows, n = _series_args(x)
        return _batched_probs(probs, rows, lambda pj, oj: _abi.check(self.lib, self.lib.rsf_predict_quantiles(
            self._ctx, n, rows, self._ptr(x), int(pj.size), _dp(pj), _dp(oj))))

    def psis_loo(self, series, std2, data, lpd, r_eff=1.0):
        """rsf_predict_psis_loo and rsf_predict_psis_finish: PSIS-LOO of a series (nout, n) in this engine's memory space (as
        predictive_partials(return_series=True) leaves it) with the draws' noise variances std2 (n,), the observation data
        (nout,) and lpd (nout,) of predictive_finish → dict of (nout,) arrays elpd_loo_k, pareto_k, n_tail, weight_ess and the
        totals elpd_loo, p_loo, elpd_loo_se (ddof 1, as elpd_waic_se; ArviZ uses ddof 0), k_threshold, n_high_k, max_pareto_k,
        n.  r_eff: the relative efficiency of the draws (ESS / n, e.g. from rank_diagnostics); it sets the tail length only.
        A row with at most four draws above the cutoff — also a row whose log-likelihoods are all equal, as k = 0 is when every
        std2 is equal — has pareto_k = +inf and is not smoothed (ArviZ's behaviour).  Ranks of the tail are global over the
        draws: nothing here is additive over shards, a multi-rank pool is gathered first."""
        x, s2, obs = self._in(series), self._in(std2), self._in(data)
        rows, n = _series_args(x, s2, obs)
        lpd = _host(lpd)
        if lpd.shape != (rows,):
            raise ValueError(f"lpd has shape {lpd.shape}, the series has {rows} rows")
        r_eff = float(r_eff)
        if not (np.isfinite(r_eff) and r_eff > 0.0):
            raise ValueError("r_eff is finite and > 0")
        out = np.empty((rows, len(_abi.PSIS_OUT)))
        tot = np.empty(len(_abi.PSIS_TOTALS))
        _abi.check(self.lib, self.lib.rsf_predict_psis_loo(self._ctx, n, rows, self._ptr(x), self._ptr(s2), self._ptr(obs), r_eff,
                                                           _dp(out)))
        _abi.check(self.lib, self.lib.rsf_predict_psis_finish(rows, n, _dp(out), _dp(lpd),
                                                              _dp(tot)))
        res = _rows_totals(out, tot, _abi.PSIS_OUT, _abi.PSIS_TOTALS)
        res["n"] = n
        return res

    def predictive_noise_quantiles(self, series, std2, probs, return_passes=False):
        """rsf_predict_noise_quantiles: the quantiles `probs` of the posterior predictive distribution of an OBSERVATION at
        every output time, the mixture mean_i N(y_ki, std2_i), of a series (nout, n) in this engine's memory space (as
        predictive_partials(return_series=True) leaves it) with the draws' noise variances std2 (n,) → (len(probs), nout)
        float64 on the host: the posterior predictive band, in which the data are expected to lie.  (predictive_quantiles is
        the credible band of the clean model series, which says where the ODE solution lies and is narrower by the noise.)
        Probabilities lie strictly inside (0, 1).  return_passes: also the passes the kernel made over each row (nout,) int32,
        at most PREDICT_NOISE_MAX_PASSES (the largest over the batches of PREDICT_MAX_PROBS probabilities).  A probability's
        result does not depend on which others are asked with it.  F is a mean over all draws: a multi-rank pool is gathered first."""
        probs = _probs(probs, True, False, "probs")
        x, s2 = self._in(series), self._in(std2)
        rows, n = _series_args(x, s2)
        passes = np.zeros(rows, dtype=np.int32)

        def call(pj, oj):
            ps = np.empty(rows, dtype=np.int32)
            _abi.check(self.lib, self.lib.rsf_predict_noise_quantiles(self._ctx, n, rows, self._ptr(x), self._ptr(s2), int(pj.size), _dp(pj),
                                                                      _dp(oj), _i32p(ps)))
            np.maximum(passes, ps, out=passes)

        out = _batched_probs(probs, rows, call)
        return (out, passes) if return_passes else out

    def predictive(self, q, std2, data, probs=(), center=None, return_series=False, loo=False, r_eff=1.0, noise_probs=()):
        """Posterior predictive checks of n draws against the observation `data`: per output time the model series' mean and
        variance over the draws, the probability integral transform of the observation (pit), the log pointwise predictive
        density (lpd) and the WAIC penalty (p_waic_k); the totals mean_std2, elpd_waic, p_waic, elpd_waic_se; with `probs` the
        exact quantiles (len(probs), nout) of the series over the draws, the credible band.  center = (center_y, center_l)
        (default: the series at the draws' mean parameter vector, and its log density with the mean sigma^2).  With probs or
        return_series the series (nout, n) is materialised: n * nout * 8 bytes.  loo=True materialises it as well and adds
        psis_loo's entries (with r_eff) to the result; the default leaves the result as it is without.
        Two bands: `quantiles` (from probs) is the CREDIBLE band of the model series — where the clean ODE solution lies;
        `noise_quantiles` (from noise_probs, each strictly inside (0, 1); see predictive_noise_quantiles) is the POSTERIOR
        PREDICTIVE band — where an observation lies, the inferred noise included: the one to overlay on the data.  A non-empty
        noise_probs materialises the series and adds the keys noise_probs and noise_quantiles; the default adds nothing."""
        return self._predictive(self.predictive_partials, lambda dc, a, b: self.forward(dc, a=a, b=b)[1], False, q, std2, data, probs, center,
                                return_series, loo, r_eff, noise_probs)

    def _predictive(self, partials, solve, law_aware, q, std2, data, probs, center, return_series, loo, r_eff, noise_probs, stiff_aware=False):
        """predictive's and law_predictive's body; partials: predictive_partials or law_predictive_partials behind its law,
        solve(dc, a, b): the series (nout, 1) at one point, for the default centre"""
        q, std2, data, n, d = self._predict_args(q, std2, data, law_aware, stiff_aware)
        probs, noise_probs = _probs(probs, False, True, "probs"), _probs(noise_probs, True, True, "noise_probs")

        if center is None:
            qm = _host(q.mean(0)).reshape(d)
            cy = _host(solve(qm[:1], qm[1:2] if d == 3 else None, qm[2:3] if d == 3 else None)).reshape(self.nout)
            ms = float(_host(std2).mean())
            cl = -0.5 * np.log(2.0 * np.pi * ms) - (_host(data) - cy) ** 2 / (2.0 * ms)
            if not (np.isfinite(cy).all() and np.isfinite(cl).all()):
                raise ValueError("the series at the draws' mean parameters is not finite; pass center=(center_y, center_l)")
        else:
            cy, cl = center
        cy, cl = self._predict_centers(cy, cl)
        want_series = bool(return_series) or probs.size > 0 or bool(loo) or noise_probs.size > 0
        part = partials(q, std2, data, cy, cl, return_series=want_series)
        series = None
        if want_series:
            part, series = part
        res = self.predictive_finish(part, cy, cl)
        res.update(partials=part, center_y=cy, center_l=cl)
        if probs.size:
            res["probs"], res["quantiles"] = probs, self.predictive_quantiles(series, probs)
        if loo:
            res.update({name: v for name, v in self.psis_loo(series, std2, data, res["lpd"], r_eff=r_eff).items() if name != "n"})
        if noise_probs.size:
            res["noise_probs"], res["noise_quantiles"] = noise_probs, self.predictive_noise_quantiles(series, std2, noise_probs)
        if return_series:
            res["series"] = series
        return res

    # -- the same checks under either state law and any observable (include/rsf_law_predict.h) -----------
    def _law_predict_fn(self, name):
        """a function of include/rsf_law_predict.h, which librsf_hip.so alone exports"""
        try:
            return getattr(self.lib, name)
        except AttributeError:
            raise _abi.RsfError(-5, f"{name} is exported by librsf_hip.so only: the {self.lib.rsf_backend().decode()!r} library has no such "
                                    "symbol (include/rsf_law_predict.h)") from None

    def law_predictive_partials(self, law, observable, q, std2, data, center_y, center_l, return_series=False):
        """rsf_law_predict_partials: predictive_partials — its arguments, checks and results — with the solve under the state law
        `law` and y the series of `observable` (law_observe's names, aliases or integers; its series bit for bit), under the loading
        table in use.  data is a series of the same observable."""
        self._need_model(law_aware=True)
        law, observable = self._law_codes(law, observable)
        return self._partials(lambda *a: self._law_predict_fn("rsf_law_predict_partials")(self._ctx, law, observable, *a), True, q, std2, data,
                              center_y, center_l, return_series)

    def series_partials(self, series, std2, data, center_y, center_l):
        """rsf_predict_series_partials: predictive_partials' partials of a series (nout, n) that exists (law_observe's, or any), in
        this engine's memory space with std2 (n,) and data (nout,), about the centres center_y, center_l (nout,) → (PREDICT_HEAD +
        nout * len(PREDICT_FIELDS),) float64 on the host, bit for bit what law_predictive_partials returns for the draws that gave
        the series.  Needs no model."""
        x, s2, obs = self._in(series), self._in(std2), self._in(data)
        rows, n = _series_args(x, s2, obs)
        cy, cl = self._predict_centers(center_y, center_l, rows)
        out = np.empty(_abi.PREDICT_HEAD + rows * len(_abi.PREDICT_FIELDS))
        _abi.check(self.lib, self._law_predict_fn("rsf_predict_series_partials")(self._ctx, n, rows, self._ptr(x), self._ptr(s2), self._ptr(obs),
                                                                                 _dp(cy), _dp(cl), _dp(out)))
        return out

    def law_predictive(self, law, observable, q, std2, data, probs=(), center=None, return_series=False, loo=False, r_eff=1.0, noise_probs=()):
        """predictive — its arguments, checks and result, key for key — for a model under the state law `law` whose data is a series
        of `observable` (law_observe's names, aliases or integers), under the loading table in use: the fused solve and reduction is
        rsf_law_predict_partials, the default centre the series of one law_observe call at the draws' mean point, and the
        quantiles, the PSIS-LOO entries and noise_quantiles come from the series entry points predictive uses.  A model with a
        stiffness independent of Dc (set_model) runs the split route: law_observe's series of every draw (rsf_stiff_observe), then
        series_partials on it — the fused kernel integrates k' = 0.1 / Dc."""
        self._need_model(law_aware=True, stiff_aware=True)
        law, observable = self._law_codes(law, observable)
        stiff = self._stiffness(None) is not None

        def centre(dc, a, b):
            # a library without this family is refused under its name, before any solve
            self._law_predict_fn("rsf_predict_series_partials" if stiff else "rsf_law_predict_partials")
            return self.law_observe(law, observable, dc, a, b)[1]

        def split(q, std2, data, center_y, center_l, return_series=False):
            q, std2, data, n, d = self._predict_args(q, std2, data, True, True)
            ab = [q[:, p] for p in (1, 2)] if d == 3 else [None, None]
            series = self.law_observe(law, observable, q[:, 0], ab[0], ab[1])[1]
            out = self.series_partials(series, std2, data, center_y, center_l)
            return (out, series) if return_series else out

        fused = lambda *a, **kw: self.law_predictive_partials(law, observable, *a, **kw)
        return self._predictive(split if stiff else fused, centre, True, q, std2, data, probs, center, return_series, loo, r_eff, noise_probs,
                                stiff_aware=True)

    # -- multi-GPU posterior pool through the C ABI (RCCL bound inside the library) -----
    def comm_unique_id(self):
        """Rank 0: the 128-byte id every rank passes to comm_init (send it over any channel)."""
        buf = (ctypes.c_uint8 * 128)()
        _abi.check(self.lib, self.lib.rsf_comm_unique_id(buf))
        return bytes(buf)

    def comm_init(self, world, rank, unique_id=None):
        """Collective: create this ctx's communicator (world = 1 needs no id)."""
        buf = (ctypes.c_uint8 * 128)(*unique_id) if unique_id is not None else None
        _abi.check(self.lib, self.lib.rsf_comm_init(self._ctx, int(world), int(rank), buf))
        self.world, self.rank = int(world), int(rank)

    def comm_destroy(self):
        _abi.check(self.lib, self.lib.rsf_comm_destroy(self._ctx))
        self.world = 0

    def pool_allgather(self, local):
        """local: array/tensor of any shape in this engine's memory space → (world,) + shape on every rank."""
        if not self.world:
            raise _abi.RsfError(-3, "pool_allgather: call comm_init first")
        x = self._in(local)
        out = self._empty((self.world,) + tuple(x.shape))
        n = int(np.prod(x.shape))
        _abi.check(self.lib, self.lib.rsf_pool_allgather(self._ctx, self._ptr(x), n, self._ptr(out)))
        return out

    def pool_allreduce_sum(self, buf):
        """In-place element-wise sum over ranks of a float64 array/tensor in this engine's memory space."""
        if not self.world:
            raise _abi.RsfError(-3, "pool_allreduce_sum: call comm_init first")
        x = self._in(buf)
        _abi.check(self.lib, self.lib.rsf_pool_allreduce_sum(self._ctx, self._ptr(x), int(np.prod(x.shape))))
        return x

    # -- the same exchange driven by ONE host thread that owns several engines (one per GPU): SURVEY §8e's process model --
    @staticmethod
    def _ctx_array(engines):
        if not engines:
            raise ValueError("need at least one engine")
        lib = engines[0].lib
        if any(e.lib is not lib for e in engines):
            raise ValueError("all engines of a group must come from the same library")
        return lib, (ctypes.c_void_p * len(engines))(*[e._ctx for e in engines])

    @staticmethod
    def comm_init_all(engines):
        """rsf_comm_init_all: engines[i] becomes rank i of a len(engines)-rank group (ncclCommInitAll; no id, no launcher)."""
        lib, ctxs = Engine._ctx_array(engines)
        _abi.check(lib, lib.rsf_comm_init_all(ctxs, len(engines)))
        for r, e in enumerate(engines):
            e.world, e.rank = len(engines), r

    @staticmethod
    def pool_allgather_all(engines, locals_):
        """One grouped all-gather: locals_[r] (same shape on every rank, in engines[r]'s memory space) → list of
        (world,) + shape arrays, one per engine, each holding every rank's block."""
        lib, ctxs = Engine._ctx_array(engines)
        n = len(engines)
        xs = [e._in(x) for e, x in zip(engines, locals_)]
        if len(xs) != n or any(tuple(x.shape) != tuple(xs[0].shape) for x in xs):
            raise ValueError("one block of the same shape per engine")
        outs = [e._empty((n,) + tuple(xs[0].shape)) for e in engines]
        send = (ctypes.c_void_p * n)(*[Engine._ptr(x) for x in xs])
        recv = (ctypes.c_void_p * n)(*[Engine._ptr(o) for o in outs])
        _abi.check(lib, lib.rsf_pool_allgather_all(ctxs, n, send, int(np.prod(xs[0].shape)), recv))
        return outs

    @staticmethod
    def pool_allreduce_sum_all(engines, bufs):
        """One grouped in-place sum over ranks: bufs[r] lives in engines[r]'s memory space → the summed buffers."""
        lib, ctxs = Engine._ctx_array(engines)
        n = len(engines)
        xs = [e._in(x) for e, x in zip(engines, bufs)]
        if len(xs) != n or any(tuple(x.shape) != tuple(xs[0].shape) for x in xs):
            raise ValueError("one buffer of the same shape per engine")
        ptrs = (ctypes.c_void_p * n)(*[Engine._ptr(x) for x in xs])
        _abi.check(lib, lib.rsf_pool_allreduce_sum_all(ctxs, n, ptrs, int(np.prod(xs[0].shape))))
        return xs

    def mcmc_adapt(self, window, adapt_mode, prior_len=0):
        """MCMC.update_covariance_matrix for one window of samples (n, d) on the device (rsf_mcmc_adapt) → the (d, d) matrix
        the reference's loop would assign to Vold; raises RsfError(-1) where np.linalg.cholesky would raise."""
        w = np.ascontiguousarray(window, dtype=np.float64)
        w = w.reshape(w.shape[0], -1)
        n, d = w.shape
        out = np.empty((d, d))
        mode = _abi.ADAPT_MODES[adapt_mode] if isinstance(adapt_mode, str) else int(adapt_mode)
        _abi.check(self.lib, self.lib.rsf_mcmc_adapt(d, n, w.ctypes.data, mode, int(prior_len), out.ctypes.data))
        return out

    # -- RNG helpers (tests) --------------------------------------------------------------
    def philox(self, ctr, key):
        c, k, o = (ctypes.c_uint32 * 4)(*ctr), (ctypes.c_uint32 * 2)(*key), (ctypes.c_uint32 * 4)()
        _abi.check(self.lib, self.lib.rsf_philox4x32_10(c, k, o))
        return list(o)

    def draws(self, seed, chain, iteration, n_params, shape):
        z, u, g = (ctypes.c_double * 3)(), ctypes.c_double(), ctypes.c_double()
        _abi.check(self.lib, self.lib.rsf_mcmc_draws(seed, chain, iteration, n_params, shape, z, ctypes.byref(u), ctypes.byref(g)))
        return list(z)[:n_params], u.value, g.value
