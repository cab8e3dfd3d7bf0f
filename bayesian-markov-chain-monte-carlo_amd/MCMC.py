"""
MCMC — drop-in for the reference sampler class (MCMC.py:4-544) with the hot loop on the GPU.

`MCMC(model, data, dc_true, qpriors, qstart, nsamples, lstm_model, adapt_interval, verbose)` and
`.sample(MAKE_ANIMATIONS)` keep the reference's signatures, return shapes and quirk modes
(SURVEY Appendix A).  Each iteration — propose, box test, forward solve, sum of squares,
accept/reject, inverse-gamma σ² update, adaptation — executes in the fused HIP kernel
(rsf_mcmc_replay / rsf_mcmc_run); the host only feeds random variates.

`sample()` draws those variates from the *global NumPy RNG in the reference's order*
(MCMC.py:497, 331, 160 and the N unused normals of every RateStateModel.evaluate call,
RateStateModel.py:392), so `np.random.seed(s)` selects the same chain the reference would run.
`sample_batched()` (additive) runs many independent chains per launch with the on-device
Philox stream and is the throughput path.

The model contract is the reference's (MCMC.py:65-66, 127, 381-384): ANY object with a settable `.Dc`
and `.evaluate()` whose second element is the clean series.  This package's RateStateModel is integrated
on the device inside the fused kernel; for any other model the host calls `model.evaluate()` where the
reference would and the device runs the chain step on the sum of squares it is handed
(rsf_mcmc_init_state / rsf_mcmc_propose / rsf_mcmc_replay_ssq).
"""
import contextlib
import math

import numpy as np

if __package__:
    from . import _figures
    from ._abi import ADAPT_MODES, ERR_NOT_POSDEF, RsfError
    from .engine import Engine, _host, bayes_factor, check_law_options, law_name, observable_of, state_law_of, stiffness_of, whole_islands  # noqa: F401
else:  # flat layout: this directory on sys.path, the reference's own import style (main.py:44-46)
    import _figures
    from _abi import ADAPT_MODES, ERR_NOT_POSDEF, RsfError
    from engine import Engine, _host, bayes_factor, check_law_options, law_name, observable_of, state_law_of, stiffness_of, whole_islands  # noqa: F401


@contextlib.contextmanager
def _engine_for(engine, model=None, substeps=None):
    """`engine`, or a host-memory Engine made for the block and closed after it; `model` is set on whichever it is, with
    `substeps` RK4 steps per output interval (by default the model's own)."""
    with Engine(mem="host") if engine is None else contextlib.nullcontext(engine) as eng:
        if model is not None:
            eng.set_model(model, int(getattr(model, "substeps", 1) if substeps is None else substeps))
        yield eng


class PosteriorPool:
    """Result of sample_batched: kept draws of every chain, iteration-major."""

    def __init__(self, samples, std2, accept_rate, stats, nburn, superchain_size=None):
        self.samples = samples          # (n_keep, C, d)
        self.std2 = std2                # (n_keep, C)
        self.accept_rate = accept_rate  # accepted / proposals over all chains
        self.stats = stats
        self.nburn = nburn
        self.superchain_size = superchain_size  # chains [k*S, (k+1)*S) started from one point (sample_batched)

    def diagnostics(self, superchain_size=None, engine=None, **kw):
        """Split R-hat, nested R-hat and multi-chain ESS of the kept draws, computed on the GPU (Engine.diagnostics) → one dict
        per parameter.  Nested R-hat uses superchains of `superchain_size` chains, by default the sampler's own."""
        S = self.superchain_size if superchain_size is None else superchain_size
        with _engine_for(engine) as eng:
            return eng.diagnostics(self.samples, superchain_size=S, **kw)

    def rank_diagnostics(self, engine=None, **kw):
        """Rank-normalised R-hat, bulk and tail ESS, median, quantiles and HDI of the kept draws, computed on the GPU
        (Engine.rank_diagnostics) → one dict per parameter.  Ranks are global: a multi-rank pool is gathered first."""
        with _engine_for(engine) as eng:
            return eng.rank_diagnostics(self.samples, **kw)

    def loo(self, model, data, max_draws=None, engine=None, substeps=None, r_eff=1.0):
        """PSIS-LOO of the kept draws against the observation `data`, computed on the GPU (Engine.predictive(loo=True)): the
        entries of predictive() without a band, and per output time elpd_loo_k, pareto_k, n_tail, weight_ess with the totals
        elpd_loo, p_loo, elpd_loo_se, k_threshold, n_high_k, max_pareto_k.  The series is materialised (n * nout * 8 bytes):
        max_draws takes an evenly strided subset as in predictive().  r_eff: the draws' relative efficiency (ESS / n, e.g.
        from rank_diagnostics).  Ranks of the tail are global: a multi-rank pool is gathered first."""
        return self.predictive(model, data, probs=(), max_draws=max_draws, engine=engine, substeps=substeps, loo=True, r_eff=r_eff)

    def predictive(self, model, data, probs=(0.05, 0.5, 0.95), max_draws=None, engine=None, substeps=None, loo=False, r_eff=1.0,
                   noise_probs=()):
        """Posterior predictive checks of the kept draws against the observation `data`, computed on the GPU (Engine.predictive):
        the draws are mapped back through `model`'s ODE (float64 RK4, `substeps` steps per output interval — by default the
        model's own) → dict with, per output time, mean, var, pit, lpd, p_waic_k and the quantiles `probs` of the model series
        (the credible band), and the totals elpd_waic, p_waic, elpd_waic_se, mean_std2.  max_draws: use an evenly strided subset
        of at most that many draws (deterministic; the band materialises n * nout * 8 bytes).  engine: an Engine to run on (its
        model is set here); by default a host-memory engine made for the call.  loo=True adds the PSIS-LOO entries (see loo).
        `quantiles` is the credible band of the clean model series; it does not contain the noise, and most observations lie
        outside it when the posterior is tight.  noise_probs (each strictly inside (0, 1)) adds `noise_quantiles`, the posterior
        predictive band of an observation — the quantiles of mean_i N(y_ik, std2_i) — which is the band to overlay on the data."""
        q, s2 = self._draws(max_draws)
        extra = dict(loo=True, r_eff=r_eff) if loo else {}  # without loo or noise_probs the engine is called as it always was
        if np.size(noise_probs):
            extra["noise_probs"] = noise_probs
        with _engine_for(engine, model, substeps) as eng:
            return eng.predictive(q, s2, data, probs=probs, **extra)

    def _draws(self, max_draws):
        """(q (m, d), std2 (m,)) on the host: every kept draw, or the evenly strided subset of at most max_draws of them"""
        n, C, d = self.samples.shape
        q, s2 = _host(self.samples).reshape(n * C, d), _host(self.std2).reshape(n * C)
        if max_draws is not None:
            if int(max_draws) < 1:
                raise ValueError("max_draws must be >= 1")
            if int(max_draws) < n * C:
                idx = (np.arange(int(max_draws), dtype=np.int64) * (n * C)) // int(max_draws)  # evenly strided, no RNG
                q, s2 = q[idx], s2[idx]
        return q, s2

    def law_predictive(self, model, data, probs=(0.05, 0.5, 0.95), max_draws=None, engine=None, substeps=None, loo=False, r_eff=1.0,
                       noise_probs=()):
        """predictive — its arguments and its result — for ANY device model (Engine.law_predictive): the state law
        (model.state_law: "aging" or "slip"), the observable `data` is a series of (model.observable: "acc", "mu", "theta" or
        "velocity") and the loading history (model.loading) are the model's, d = 1 or 3: the checks of a pool that sample_law
        returned.  The result also carries `law` and `observable`, the names the solve ran under.  A model with a stiffness
        (model.stiffness) runs Engine.law_predictive's split route: law_observe's series, then series_partials."""
        q, s2 = self._draws(max_draws)
        law, observable = state_law_of(model), observable_of(model)
        extra = dict(loo=True, r_eff=r_eff) if loo else {}
        if np.size(noise_probs):
            extra["noise_probs"] = noise_probs
        with _engine_for(engine, model, substeps) as eng:
            res = eng.law_predictive(law, observable, q, s2, data, probs=probs, **extra)
        res.update(law=law, observable=observable)
        return res

    def law_loo(self, model, data, max_draws=None, engine=None, substeps=None, r_eff=1.0):
        """loo for any device model: law_predictive without a band and with the PSIS-LOO entries."""
        return self.law_predictive(model, data, probs=(), max_draws=max_draws, engine=engine, substeps=substeps, loo=True, r_eff=r_eff)

    def joint(self, engine=None):
        """Mean, covariance (ddof = 1) and correlation matrix of the kept draws over all parameters, computed on the GPU
        (Engine.pool_joint) → dict(n, nonfinite, mean (d,), cov (d, d), corr (d, d))."""
        with _engine_for(engine) as eng:
            return eng.pool_joint(self.samples)

    def corner(self, nbins=40, grid=32, probs=(0.5, 0.9), ranges=None, engine=None):
        """Everything a corner plot of the kept draws needs, computed on the GPU; drawing is the caller's.  → dict with
        joint (see joint), ranges (d, 2), probs,
        marginals: per parameter p dict(counts (nbins,) and edges (nbins + 1,) of the 1-D histogram on ranges[p], grid (grid,) and
        density (grid,) of the 1-D Gaussian KDE), and
        pairs: {(i, j): dict(counts (nbins, nbins) with xedges and yedges as numpy.histogram2d returns them for (x_i, x_j),
        x (grid,), y (grid,) and density (grid, grid) — density[k, l] at (x[k], y[l]), the 2-D Gaussian KDE — and levels, the
        highest-density contour levels of `counts` at `probs`)} for i < j.
        ranges: (d, 2) of (lo, hi) per parameter; by default each parameter's min and max, so that every draw is counted."""
        x = self.samples
        d, nbins, grid = int(x.shape[-1]), int(nbins), int(grid)
        with _engine_for(engine) as eng:
            if ranges is None:
                ranges = [(s["min"], s["max"]) for s in (eng.pool_summary(x, p) for p in range(d))]
            ranges = np.asarray(ranges, dtype=np.float64).reshape(d, 2)
            axes = [np.linspace(lo, hi, grid) for lo, hi in ranges]
            edges = [np.linspace(lo, hi, nbins + 1) for lo, hi in ranges]
            res = {"joint": eng.pool_joint(x), "ranges": ranges, "probs": np.asarray(probs, dtype=np.float64), "marginals": [], "pairs": {}}
            for p in range(d):
                res["marginals"].append({"counts": _host(eng.pool_histogram(x, nbins, ranges[p, 0], ranges[p, 1], param=p))[1:-1],
                                         "edges": edges[p], "grid": axes[p], "density": _host(eng.pool_kde(x, axes[p], param=p))})
            for i in range(d):
                for j in range(i + 1, d):
                    counts = _host(eng.pool_histogram2d(x, nbins, (ranges[i], ranges[j]), params=(i, j)))[1:-1, 1:-1]
                    mesh = np.stack(np.meshgrid(axes[i], axes[j], indexing="ij"), axis=-1).reshape(grid * grid, 2)
                    res["pairs"][i, j] = {"counts": counts, "xedges": edges[i], "yedges": edges[j], "x": axes[i], "y": axes[j],
                                          "density": _host(eng.pool_kde2d(x, mesh, params=(i, j))).reshape(grid, grid),
                                          "levels": eng.pool_hpd_levels(counts, probs)}
        return res

    def evidence(self, model, data, lo, hi, transform=None, engine=None, substeps=None, **kw):
        """The marginal likelihood p(data | model) of the fit these draws came from, by bridge sampling on the GPU
        (Engine.evidence): the kept trace, sampled with n0 = 0 inside the box (lo, hi), is split along the iterations; the
        effective sample size of the second part comes from the diagnostics.  → Engine.evidence's dict; two fits of one data
        set compare with bayes_factor.  transform: per parameter "identity" or "log" (log needs lo > 0); by default the identity
        for every parameter, also for (Dc, a, b): measured on the two fits of DESIGN.md 4g, log on (Dc, a) brings no more proposal
        draws into the box (0.977 both) and an re of 5.9e-3 against 6.8e-3, and it would refuse the usual box, whose Dc starts at 0."""
        with _engine_for(engine, model, substeps) as eng:
            return eng.evidence(self.samples, data, lo, hi, transform=transform, **kw)

    def law_evidence(self, model, data, lo, hi, transform=None, engine=None, substeps=None, **kw):
        """evidence — its arguments and its result — for ANY device model (Engine.law_evidence): the state law, the observable
        `data` is a series of and the loading history are the model's, d = 1 or 3: the marginal likelihood of a pool that
        sample_law or LawGridPosterior.pool returned.  The result also carries `law` and `observable`."""
        law, observable = state_law_of(model), observable_of(model)
        if stiffness_of(model) is not None:
            raise NotImplementedError(f"PosteriorPool.law_evidence cannot run a model with stiffness={stiffness_of(model)!r}: the kernel "
                                      "integrates k' = 0.1 / Dc (Engine.law_logtarget); sample_smc and quadrature (d = 1) give its evidence")
        with _engine_for(engine, model, substeps) as eng:
            res = eng.law_evidence(law, observable, self.samples, data, lo, hi, transform=transform, **kw)
        res.update(law=law, observable=observable)
        return res

    def pooled(self):
        """(d, n_keep*C): every kept draw of every chain, the reference's (d, n) layout."""
        n, C, d = self.samples.shape
        return np.ascontiguousarray(self.samples.reshape(n * C, d).T)


class MCMC:
    def __init__(self, model, data, dc_true, qpriors, qstart, nsamples=100, lstm_model={}, adapt_interval=10,
                 verbose=True):
        self.model = model
        self.qstart = qstart
        self.qpriors = qpriors
        self.nsamples = nsamples
        self.nburn = int(nsamples / 2)
        self.verbose = verbose
        self.adapt_interval = adapt_interval
        self.data = data
        self.lstm_model = lstm_model
        self.n0 = 0.01
        if self._multi_parameter():
            # additive (BASELINE config 5): joint (Dc, a, b) — one ["Uniform", lo, hi] spec per parameter, qstart a 3-vector.  The
            # reference's sampler has one parameter (MCMC.py:98, 381); the three-parameter chains run through sample_batched only.
            if len(self.qpriors) != 3 or np.size(self.qstart) != 3:
                raise ValueError("joint inference takes three prior specs [[name, lo, hi]] x 3 for (Dc, a, b) and a 3-vector qstart")
            self.qstart_limits = np.array([[p[1], p[2]] for p in self.qpriors], dtype=np.float64)
        else:
            self.qstart_limits = np.array([[self.qpriors[1], self.qpriors[2]]])
        self.dc_true = dc_true
        # additive: consume the N normals each reference forward solve wastes (RateStateModel.py:392)
        self.replay_reference_rng = True

    # ---- helpers ------------------------------------------------------------------------
    def _device_model(self):
        """True: the model is this package's RateStateModel, integrated on the device inside the sampler kernel.
        False: any other object with `.Dc` and `.evaluate()` — the host evaluates it, the device runs the chain step."""
        return hasattr(self.model, "engine")

    def _engine(self):
        if self.lstm_model:
            raise NotImplementedError("the reduced-order-model hook (MCMC.py:124-125) has no implementation "
                                      "in the reference either; pass a falsy lstm_model")
        if self._device_model():
            return self.model.engine()
        if getattr(self, "_host_engine", None) is None:
            self._host_engine = Engine(mem="host")  # no set_model: the chain logic alone (rsf_mcmc_init_state)
        return self._host_engine

    def _prior_is_dict(self):
        return hasattr(self.qpriors, "keys")

    def _multi_parameter(self):
        """Three prior specs, one per parameter of (Dc, a, b), instead of the reference's single ["Uniform", lo, hi]."""
        try:
            first = self.qpriors[0]
        except (KeyError, IndexError, TypeError):
            return False
        return not isinstance(first, (str, bytes)) and np.ndim(first) == 1 and len(first) == 3

    @property
    def n_params(self):
        return 3 if self._multi_parameter() else 1

    def _adapt_mode(self):
        # list prior: update_covariance_matrix raises AttributeError, swallowed at MCMC.py:524-527 => never adapts.
        # Three parameters (this build's extension): corrected adaptive Metropolis — the initial proposal follows the (Dc, a)
        # ridge only locally, and what the chains learn about it is what makes them mix
        if self._multi_parameter():
            return "am"
        return "reference_dict" if self._prior_is_dict() else "none"

    def _law(self):
        """the model's state evolution law, "aging" or "slip" """
        return state_law_of(self.model)

    def _observable(self):
        """the series the model returns and `data` holds: "acc", "mu", "theta" or "velocity" """
        return observable_of(self.model)

    def _split(self):
        """None, or what sends the model through the plain solve's sums of squares (Engine.law_ssq_fn) in place of the fused
        kernels, which integrate the ageing law and fit the acceleration: the slip law, or another observable under either law"""
        if self._law() == "slip":
            return "state_law='slip'"
        if self._observable() != "acc":
            return f"observable={self._observable()!r}"
        return None if self._stiffness() is None else f"stiffness={self._stiffness()!r}"

    def _stiffness(self):
        """the model's stiffness independent of Dc, or None for the reference's coupling k' = 0.1 / Dc"""
        return stiffness_of(self.model)

    def _ssq_fn(self, eng, data):
        return eng.law_ssq_fn(self._law(), data, observable=self._observable())  # the engine's model's stiffness, if it has one

    def _coupled_only(self, what):
        """`what` runs kernels that integrate the reference's spring: refuse a model with a stiffness of its own"""
        if self._stiffness() is not None:
            raise NotImplementedError(f"{what} cannot run a model with stiffness={self._stiffness()!r}: the kernel integrates k' = 0.1 / Dc; "
                                      "with a stiffness quadrature (d = 1), compare_laws, sample_smc, sample_dr, sample_law, fit_law and "
                                      "SSqcalc run")

    def _ageing_only(self, what):
        """`what` runs kernels that integrate the ageing law: refuse a model with another law instead of running the ageing law"""
        self._coupled_only(what)
        if self._law() != "aging":
            raise NotImplementedError(f"{what} integrates the ageing law only and the model's state_law is {self._law()!r}: under the slip "
                                      "law quadrature, compare_laws, sample_smc and sample_dr run")
        if self._observable() != "acc":
            raise NotImplementedError(f"{what} fits the acceleration only and the model's observable is {self._observable()!r}: on another "
                                      "observable quadrature, compare_laws, sample_smc, sample_dr and SSqcalc run")

    def _init_chains(self, eng, q0, seed=0, chain_offset=0, adapt_mode=None):
        self._ageing_only("the fused sampler (sample, sample_batched and the reference's sub-methods)")
        data = np.ascontiguousarray(self.data, dtype=np.float64).reshape(-1)
        lo, hi = self.qstart_limits[:, 0], self.qstart_limits[:, 1]
        # forward-difference step of the initial sensitivities: the reference's 1e-6 for its one parameter (MCMC.py:251); 1e-4 for
        # the three-parameter extension, whose regularised covariance does not need the small step and is cleaner without it
        eng.mcmc_init(q0, data, lo, hi, seed=seed, chain_offset=chain_offset, n0=self.n0,
                      prior_len=len(self.qpriors), adapt_mode=adapt_mode or self._adapt_mode(),
                      adapt_interval=self.adapt_interval, fd_rel_step=1e-4 if self._multi_parameter() else 1e-6)

    # ---- reference sub-methods (public names kept; each one runs its step on the device) -----------------------
    # A caller that composes them the way the reference's own loop does (MCMC.py:494-527) gets the arithmetic of the fused
    # kernel: acceptreject and update_standard_deviation are one replayed kernel iteration on the engine's chain,
    # update_covariance_matrix the kernel's adaptation step on the given window.  The variates come from NumPy's global
    # stream in the reference's order, exactly as in sample().
    def evaluate_model(self):
        if self.lstm_model:
            raise NotImplementedError("reduced-order-model hook: no such class exists in the reference")
        return self.model.evaluate()[1]

    def SSqcalc(self, q_new):
        """Sum of squares at q_new (d, 1) → (1, 1) (MCMC.py:381-387); one GPU forward solve — or, for a model that is not
        this package's RateStateModel, one `model.evaluate()` on the host."""
        self.model.Dc = q_new[0, ]
        if not self._device_model():
            acc = np.asarray(self.evaluate_model(), dtype=np.float64)
            return np.sum((acc.reshape(1, -1) - np.asarray(self.data, dtype=np.float64).reshape(1, -1)) ** 2, axis=1, keepdims=True)
        eng = self._engine()
        dc = float(np.asarray(self.model.Dc, dtype=np.float64).reshape(-1)[0])
        if self._split():
            return self._ssq_fn(eng, np.asarray(self.data, dtype=np.float64).reshape(-1))([[dc]]).reshape(1, 1)
        ssq, _ = eng.forward([dc], data=np.asarray(self.data, dtype=np.float64).reshape(-1), want_ssq=True, want_acc=False)
        return ssq.reshape(1, 1)

    def _chain_key(self):
        # the chain on the engine belongs to THIS sampler and THIS observation: a different `data` array means new chains
        return (id(self), id(self.data), len(self.data))

    def _scratch_chain(self, eng):
        """The engine's one-chain sampler state the sub-methods work on (created by compute_initial_covariance, or here)."""
        if eng.n_chains != 1 or eng.n_params != 1 or getattr(eng, "_chain_owner", None) != self._chain_key():
            if self._device_model():
                self._init_chains(eng, np.array([[float(self.qstart)]]))
            else:  # any state will do: every sub-method sets the state it works from
                eng.mcmc_init_state([[float(self.qstart)]], [0.0], [1.0], [[[0.0]]], self.qstart_limits[:, 0], self.qstart_limits[:, 1],
                                    n0=self.n0, prior_len=len(self.qpriors), adapt_mode=self._adapt_mode(),
                                    adapt_interval=self.adapt_interval)
            eng._chain_owner = self._chain_key()
        return eng

    def _one_iteration(self, eng, q, ssq, std2, V, z, u, g, ssq_new=None):
        """One kernel iteration from an explicit chain state → (q, SSq, sigma^2, accepted) after it.  rsf_mcmc_replay (the
        kernel solves the proposal itself), or rsf_mcmc_replay_ssq when the host has evaluated the model (ssq_new)."""
        eng.set_state(q=[[q]], ssq=[ssq], std2=[std2], V=[[[V]]])
        if ssq_new is None:
            tq, ts, ta = eng.mcmc_replay(np.array([[[z]]]), np.array([[u]]), np.array([[g]]))
        else:
            tq, ts, ta = eng.mcmc_replay_ssq(np.array([[[z]]]), np.array([[u]]), np.array([[g]]), np.array([[ssq_new]]))
        return float(tq[0, 0, 0]), float(eng.get_state()[1][0]), float(ts[0, 0]), bool(ta[0, 0])

    def acceptreject(self, q_new, SSqprev, std2):
        """(accept, SSq) for the proposal q_new (MCMC.py:268-333): the kernel's box test, forward solve and accept test, with
        the uniform drawn from NumPy only when the proposal is inside the box (the reference's draw order)."""
        eng = self._scratch_chain(self._engine())
        q = float(np.asarray(q_new, dtype=np.float64).reshape(-1)[0])
        lo, hi = float(self.qstart_limits[0, 0]), float(self.qstart_limits[0, 1])
        u, ssq_new = 1.0, None
        if q > lo and q < hi:
            if not self._device_model():
                ssq_new = float(self.SSqcalc(np.asarray(q_new, dtype=np.float64).reshape(-1, 1))[0, 0])  # the model draws what it draws
            elif self.replay_reference_rng:
                np.random.randn(len(self.data))  # the N normals the reference's forward solve wastes (RateStateModel.py:392)
            u = np.random.rand()
        elif not self._device_model():
            ssq_new = 0.0  # out of bounds: never read
        # proposal = q + chol(V) z with V = 0: the kernel proposes exactly q_new from the state (q_new, SSqprev, std2)
        _, ssq, _, accept = self._one_iteration(eng, q, float(np.asarray(SSqprev).reshape(-1)[0]), float(std2), 0.0, 0.0, u, 1.0, ssq_new)
        return accept, (np.array([[ssq]]) if accept else SSqprev)

    def update_standard_deviation(self, SSqprev):
        """Appends sigma^2 ~ InvGamma(0.5 (n0 + N), 0.5 (n0 sigma^2 + SSq)) (MCMC.py:129-160) — the kernel's Gibbs step: one
        iteration whose proposal is out of bounds (z = +inf), so that nothing else of the chain moves."""
        eng = self._scratch_chain(self._engine())
        g = np.random.standard_gamma(0.5 * (self.n0 + len(self.data)))  # == gamma.rvs(aval, scale=1/bval) * bval
        _, _, s2, _ = self._one_iteration(eng, float(self.qstart), float(np.asarray(SSqprev).reshape(-1)[0]), float(self.std2[-1]),
                                          1.0, np.inf, 1.0, g, None if self._device_model() else 0.0)
        self.std2.append(s2)

    def update_covariance_matrix(self, qparams):
        """chol(2.38^2 / len(qpriors.keys()) * cov(last adapt_interval samples)) (MCMC.py:162-204), on the device.  A list
        prior has no .keys(): AttributeError, as in the reference (whose loop swallows it: the chain never adapts)."""
        n_keys = len(self.qpriors.keys())
        window = np.asarray(qparams, dtype=np.float64)[:, -self.adapt_interval:].T
        if window.shape[1] != 1:
            # the reference's np.cov / cholesky take any number of rows, but its sampler has ONE parameter (MCMC.py:98, 381) and
            # so has this quirk mode on the device; say so instead of reporting a covariance failure the caller would swallow
            raise NotImplementedError(f"update_covariance_matrix: qparams has {window.shape[1]} rows; the reference sampler and its "
                                      "dict-prior adaptation are one-parameter (corrected adaptation for 3 parameters: "
                                      "sample_batched(adapt_mode='am'))")
        try:
            return self._engine().mcmc_adapt(window, "reference_dict", prior_len=n_keys)
        except RsfError as ex:
            if ex.code == ERR_NOT_POSDEF:  # only this status is np.linalg.cholesky's failure (MCMC.py:203, 524-527)
                raise np.linalg.LinAlgError("Matrix is not positive definite") from ex
            raise

    def compute_initial_covariance(self):
        """std2[0] and Vstart (MCMC.py:244-266): from the device init kernel, or — for a model that is not this package's
        RateStateModel — from two `model.evaluate()` calls on the host, the reference's own steps."""
        if self._device_model():
            self._ageing_only("compute_initial_covariance")
        eng = self._engine()
        if self._device_model():
            self._init_chains(eng, np.array([[float(self.qstart)]]))
            eng._chain_owner = self._chain_key()
            _, _, std2, V = eng.get_state()
            self.std2 = [float(std2[0])]
            self.Vstart = V.reshape(1, 1).copy()
            self.model.Dc = self.qstart * (1 + 1e-6)  # the reference leaves the model perturbed (MCMC.py:251)
            return
        data = np.asarray(self.data, dtype=np.float64).reshape(1, -1)
        self.model.Dc = self.qstart
        acc = np.asarray(self.evaluate_model(), dtype=np.float64).reshape(1, -1)           # MCMC.py:245-248
        self.model.Dc = self.model.Dc * (1 + 1e-6)                                         # :251
        acc_dq = np.asarray(self.evaluate_model(), dtype=np.float64).reshape(1, -1)        # :254
        self.std2 = [np.sum((acc - data) ** 2, axis=1).item() / (acc.shape[1] - len(self.qpriors))]   # :261
        X = ((acc_dq - acc) / (self.model.Dc * 1e-6)).T                                    # :264, perturbed Dc in the denominator
        self.Vstart = self.std2[-1] * np.linalg.inv(X.T @ X)                               # :265-266

    # ---- the hot loop -------------------------------------------------------------------
    def sample(self, MAKE_ANIMATIONS=False):
        """One chain, nsamples proposals → ndarray (1, nsamples + 1 - nburn)  (MCMC.py:391-544)."""
        if self._multi_parameter():
            raise NotImplementedError("sample() is the reference's one-parameter loop (MCMC.py:98, 381); joint (Dc, a, b) chains run "
                                      "through sample_batched")
        if self._device_model():
            self._ageing_only("sample()")
        eng = self._engine()
        if not self._device_model():
            return self._sample_host_model(eng, MAKE_ANIMATIONS)
        N = len(self.data)
        burn = self.replay_reference_rng
        self.compute_initial_covariance()
        if burn:  # two solves in compute_initial_covariance + the initial SSqcalc
            np.random.randn(N), np.random.randn(N), np.random.randn(N)
        lo, hi = float(self.qstart_limits[0, 0]), float(self.qstart_limits[0, 1])
        aval = 0.5 * (self.n0 + N)
        qparams = np.empty((1, self.nsamples + 1))
        qparams[0, 0] = self.qstart
        std2 = list(self.std2)
        iaccept = 0
        # the host needs the current point and proposal variance only to know whether the reference would draw u
        # (in-bounds test): q follows from the trace row, V changes only where the chain adapts
        q_state, _, _, V_state = eng.get_state()
        q_cur, v_cur = float(q_state[0, 0]), float(V_state[0, 0, 0])
        adapts = self._adapt_mode() != "none"
        for isample in range(self.nsamples):
            z = np.random.standard_normal()  # the single normal multivariate_normal consumes (MCMC.py:497)
            with np.errstate(invalid="ignore"):
                q_new = q_cur + np.sqrt(v_cur) * z
            u = 1.0
            if q_new > lo and q_new < hi:  # the reference draws u only for in-bounds proposals
                if burn:
                    np.random.randn(N)
                u = np.random.rand()
            g = np.random.standard_gamma(aval)
            tq, ts, ta = eng.mcmc_replay(np.array([[[z]]]), np.array([[u]]), np.array([[g]]))
            accept = bool(ta[0, 0])
            iaccept += accept
            q_cur = float(tq[0, 0, 0])
            qparams[0, isample + 1] = q_cur
            std2.append(float(ts[0, 0]))
            if adapts and (isample + 1) % self.adapt_interval == 0:
                v_cur = float(eng.get_state()[3][0, 0, 0])
            if self.verbose:
                print(isample, accept)
                print("Generated Sample ---- ", q_new)
        if self.verbose:
            print("acceptance ratio:", iaccept / self.nsamples)
        self.std2 = np.asarray(std2)[self.nburn:]
        self.acceptance_ratio = iaccept / self.nsamples
        if MAKE_ANIMATIONS:
            self._animate(qparams)
        return qparams[:, self.nburn:]

    def _sample_host_model(self, eng, MAKE_ANIMATIONS):
        """sample() for ANY model object with `.Dc` and `.evaluate()` (the reference's contract, MCMC.py:65-66, 127): the
        host calls the model exactly where the reference does — so whatever the model draws from NumPy's global stream
        is drawn in the reference's order — and every chain step (proposal, box test, accept test, sigma^2, adaptation)
        runs on the device on the sum of squares it is handed."""
        N = len(self.data)
        self.compute_initial_covariance()                                   # MCMC.py:464
        ssq0 = float(self.SSqcalc(np.array([[float(self.qstart)]]))[0, 0])  # :468
        lo, hi = self.qstart_limits[:, 0], self.qstart_limits[:, 1]
        eng.mcmc_init_state([[float(self.qstart)]], [ssq0], [float(self.std2[-1])], np.reshape(self.Vstart, (1, 1, 1)), lo, hi,
                            n0=self.n0, prior_len=len(self.qpriors), adapt_mode=self._adapt_mode(), adapt_interval=self.adapt_interval)
        eng._chain_owner = self._chain_key()
        aval = 0.5 * (self.n0 + N)
        qparams = np.empty((1, self.nsamples + 1))
        qparams[0, 0] = self.qstart
        std2 = list(self.std2)
        iaccept = 0
        for isample in range(self.nsamples):
            z = np.array([[np.random.standard_normal()]])  # the single normal multivariate_normal consumes (MCMC.py:497)
            q_new, inb = eng.mcmc_propose(z)
            u, ssq_new = 1.0, 0.0
            if inb[0]:  # MCMC.py:322-331: the model is evaluated, then the uniform is drawn
                ssq_new = float(self.SSqcalc(q_new.reshape(-1, 1))[0, 0])
                u = np.random.rand()
            g = np.random.standard_gamma(aval)
            tq, ts, ta = eng.mcmc_replay_ssq(z.reshape(1, 1, 1), np.array([[u]]), np.array([[g]]), np.array([[ssq_new]]))
            accept = bool(ta[0, 0])
            iaccept += accept
            qparams[0, isample + 1] = float(tq[0, 0, 0])
            std2.append(float(ts[0, 0]))
            if self.verbose:
                print(isample, accept)
                print("Generated Sample ---- ", q_new.reshape(-1, 1))
        if self.verbose:
            print("acceptance ratio:", iaccept / self.nsamples)
        self.std2 = np.asarray(std2)[self.nburn:]
        self.acceptance_ratio = iaccept / self.nsamples
        if MAKE_ANIMATIONS:
            self._animate(qparams)
        return qparams[:, self.nburn:]

    def sample_batched(self, n_chains, seed=0, q0=None, jitter=None, n_iters=None, iters_per_launch=None,
                       adapt_mode=None, mem="device", device=-1, chain_offset=0, keep="post_burn", thin=1, superchain_size=None):
        """Throughput path (additive): n_chains independent chains, Philox variates on device.

        q0: (C,) / (C, d) start points; default qstart for every chain, optionally jittered
        uniformly in `jitter=(lo, hi)` with a NumPy generator seeded by `seed` and keyed by
        global chain id.  Returns a PosteriorPool of the post-burn-in draws; `thin=k` keeps every k-th kept draw
        (the pool of a long multi-GPU run need not hold, or all-gather, every iteration: SURVEY §8e).
        superchain_size=S: the jitter generator is keyed by global chain id // S instead, so that each block of S consecutive
        chains shares a start point — the superchains of nested R-hat (PosteriorPool.diagnostics)."""
        if int(thin) < 1:
            raise ValueError("thin must be >= 1")
        S = None if superchain_size is None else int(superchain_size)
        if S is not None and (S < 1 or n_chains % S or chain_offset % S):
            raise ValueError(f"superchain_size={superchain_size} must divide n_chains={n_chains} and chain_offset={chain_offset}")
        thin = int(thin)
        n_iters = self.nsamples if n_iters is None else n_iters
        nburn = int(n_iters / 2) if keep == "post_burn" else 0
        gids = chain_offset + np.arange(n_chains)
        d = self.n_params
        if q0 is None:
            q0 = np.tile(np.asarray(self.qstart, dtype=np.float64).reshape(1, d), (n_chains, 1))
            if jitter is not None:  # (lo, hi) for Dc, or one (lo, hi) per parameter: start points spread over that box
                jit = np.broadcast_to(np.asarray(jitter, dtype=np.float64).reshape(-1, 2), (d, 2)) if np.ndim(jitter) > 1 else None
                for r, g in enumerate(gids):
                    rng = np.random.default_rng([seed, int(g) if S is None else int(g) // S])
                    if jit is None:
                        q0[r, 0] = rng.uniform(*jitter)
                    else:
                        q0[r] = rng.uniform(jit[:, 0], jit[:, 1])
        q0 = np.asarray(q0, dtype=np.float64).reshape(n_chains, -1)
        if q0.shape[1] != d:
            raise ValueError(f"q0 has {q0.shape[1]} columns, the sampler {d} parameter(s)")
        if not self._device_model():
            raise TypeError("sample_batched integrates the model on the device: `model` must be this package's RateStateModel "
                            "(sample() takes any model object with .Dc and .evaluate())")
        self._ageing_only("sample_batched")
        eng = Engine(mem=mem, device=device)
        try:
            eng.set_model(self.model, getattr(self.model, "substeps", 1))
            self._init_chains(eng, q0, seed=seed, chain_offset=chain_offset, adapt_mode=adapt_mode)
            # three parameters under "am": the proposal adapts during burn-in only and is frozen from there on.  Adapting for
            # ever makes each chain's proposal depend on its own history, and the pool then misses the posterior: with n0 = 0
            # the pooled mean of `a` sat 20 standard errors below the exact target (tests/test_gpu_posterior.py)
            freeze = nburn if d == 3 and (adapt_mode or self._adapt_mode()) == "am" and 0 < nburn < n_iters else None
            earlier = None
            step = iters_per_launch or n_iters
            kept_q, kept_s, done = [], [], 0
            while done < n_iters:
                if done == freeze:
                    earlier = eng.stats()
                    state = eng.get_state()
                    # fresh Philox key for the frozen phase: its iteration count starts again at 0
                    self._init_chains(eng, state[0], seed=(int(seed) * 0x9E3779B97F4A7C15 + 1) % 2 ** 64,
                                      chain_offset=chain_offset, adapt_mode="none")
                    eng.set_state(*state)
                n = min(step, n_iters - done, (freeze - done) if freeze is not None and done < freeze else n_iters)
                tq, ts, _ = eng.mcmc_run(n, traces=("q", "std2"))
                first = max(nburn - 1 - done, 0)  # trace row r is qparams column done + r + 1
                if first < n:
                    kept_q.append(tq[first:])
                    kept_s.append(ts[first:])
                done += n
            eng.sync()
            stats = eng.stats()
            if earlier is not None:
                stats = {k: v + earlier[k] for k, v in stats.items()}
            cat = (lambda xs: np.concatenate([np.asarray(x.cpu() if hasattr(x, "cpu") else x) for x in xs], axis=0))
            samples, std2 = cat(kept_q)[::thin], cat(kept_s)[::thin]
        finally:
            eng.close()
        rate = stats["accepted"] / max(1, n_iters * n_chains)
        return PosteriorPool(samples, std2, rate, stats, nburn, superchain_size=S)

    @staticmethod
    def _smc_pool(res, extra=None):
        """One result of Engine.smc (or one run of Engine.smc_batch), its arrays on the host → the PosteriorPool of sample_smc."""
        q, std2, l = _host(res["q"]), _host(res["std2"]), _host(res["l"])
        stats = {k: res[k] for k in ("log_integral", "log_evidence", "stages", "n_solves", "shape")}
        stats["l"] = l
        stats.update(extra or {})
        rate = float(np.mean([s["accept_rate"] for s in res["stages"]]))
        rows = 16 if q.shape[0] % 16 == 0 else 1
        samples = np.ascontiguousarray(q.reshape(-1, rows, q.shape[1]).transpose(1, 0, 2))
        return PosteriorPool(samples, np.ascontiguousarray(std2.reshape(-1, rows).T), rate, stats, 0)

    def sample_smc(self, n_particles, seed=0, ess_fraction=0.5, steps=3, max_stages=200, mem="device", device=-1, offset=0, replicates=1):
        """Tempered sequential Monte Carlo (additive; Engine.smc): n_particles start uniform in the prior box and end as an
        equally weighted sample of the n0 = 0 target — no start point, no burn-in, the proposal at every stage is the population's
        own covariance.  Returns a PosteriorPool on which predictive, loo, joint, corner and evidence work unchanged.  Its layout is
        (16, n_particles / 16, d) when 16 divides n_particles — column c holds the particles 16 c .. 16 c + 15, so that the copies
        systematic resampling leaves next to each other read as the autocorrelation of one column, which is where evidence's ESS
        factor looks for it — and (1, n_particles, d) otherwise (evidence then needs a flat pool and fit_fraction).  Its stats carry log_integral, log_evidence (the constants of Engine.evidence_finish), the stage table
        `stages`, n_solves and the particles' l = -shape log SSq.  accept_rate is the mean over the stages' Metropolis steps.
        replicates > 1: that many independent populations, seeds seed .. seed + replicates - 1, run together (Engine.smc_batch);
        the pool is the first one's — the run replicates = 1 gives — and its stats add replicate_log_evidence, the replicates'
        log evidences, log_evidence_mean (the logarithm of their mean evidence) and log_evidence_se, its standard error: the error
        bar one run's dependent particles cannot give."""
        if not self._device_model():
            raise TypeError("sample_smc integrates the model on the device: `model` must be this package's RateStateModel")
        data = np.ascontiguousarray(self.data, dtype=np.float64).reshape(-1)
        lo, hi = self.qstart_limits[:, 0], self.qstart_limits[:, 1]
        with Engine(mem=mem, device=device) as eng:
            eng.set_model(self.model, getattr(self.model, "substeps", 1))
            if self._split():  # the split path: the GPU's weights, resampling, proposals and accept tests on the plain solve's SSq
                if int(replicates) > 1:
                    self._coupled_only("sample_smc(replicates > 1)")
                    raise NotImplementedError("sample_smc(replicates > 1) runs the batched kernels, which integrate the ageing law; the model's "
                                              "state_law is 'slip'" if self._law() == "slip" else
                                              f"sample_smc(replicates > 1) runs the batched kernels, which fit the acceleration; the model's {self._split()}")
                res = eng.smc_from_ssq(self._ssq_fn(eng, data), lo, hi, int(n_particles), 0.5 * eng.nout, seed=seed, offset=offset,
                                       ess_fraction=ess_fraction, steps=steps, max_stages=max_stages)
                eng.sync()
                return self._smc_pool(res)
            if int(replicates) > 1:
                out = eng.smc_batch(data, lo, hi, int(n_particles), seeds=int(seed), offsets=int(offset), replicates=int(replicates),
                                    ess_fraction=ess_fraction, steps=steps, max_stages=max_stages)
                eng.sync()
                summ = out["summary"][0]
                return self._smc_pool(out["runs"][0], {"replicate_log_evidence": np.array([r["log_evidence"] for r in out["runs"]]),
                                                       "log_evidence_mean": summ["log_evidence_mean"], "log_evidence_se": summ["log_evidence_se"]})
            res = eng.smc(data, lo, hi, int(n_particles), seed=seed, offset=offset, ess_fraction=ess_fraction, steps=steps, max_stages=max_stages)
            eng.sync()
            return self._smc_pool(res)

    @staticmethod
    def _mala_pool(res, std2, nburn, extra=None):
        """Engine.mala's result and the kept states' sigma^2 → the PosteriorPool of sample_mala"""
        stats = {"accepted": int(res.accepted.sum()), "out_of_bounds": int(res.outbox.sum()), "stuck": int(res.stuck.sum()),
                 "evaluated": int(res.n_iter * res.accepted.shape[0] - res.outbox.sum() - res.stuck.sum()), "n_iter": res.n_iter,
                 "shape": res.shape, "ssq": res.ssq_trace}
        stats.update(extra or {})
        return PosteriorPool(res.samples, std2, res.accept_rate, stats, nburn)

    def sample_mala(self, n_chains, n_iter, nburn=None, start="fit", seed=0, eps=1.0, lam=1e-3, mem="device", device=-1, chain_offset=0, thin=1):
        """Gauss-Newton manifold MALA (additive; Engine.mala): n_chains chains whose proposal is rebuilt in every iteration from
        the normal equations at the chain's point — no proposal covariance, no adaptation, an exact Metropolis-Hastings
        correction; each iteration is one group solve of 1 + d trajectories.  The target is the n0 = 0 posterior
        pi(q) ~ 1_box SSq^-N/2, sigma^2 drawn afterwards from its conditional.  start="fit": every chain starts at
        self.fit(seed=seed).best()'s point; start="qstart": at qstart; chains started at one point are independent through their
        Philox streams (seed, chain_offset + i).  nburn: iterations dropped, by default n_iter // 2; every thin-th of the others is
        kept.  Returns a PosteriorPool (samples (n_keep, n_chains, d), std2, accept_rate) on which diagnostics, rank_diagnostics,
        predictive, loo, joint, corner and evidence work unchanged; its stats carry the proposals accepted, out_of_bounds and stuck
        (no proposal: the metric did not factor), evaluated, the group solves spent, and the kept states' ssq."""
        n_chains, n_iter = int(n_chains), int(n_iter)
        nburn = n_iter // 2 if nburn is None else int(nburn)
        if n_chains < 1 or n_iter < 1 or not 0 <= nburn < n_iter or int(thin) < 1:
            raise ValueError("n_chains >= 1, n_iter >= 1, 0 <= nburn < n_iter, thin >= 1")
        if start not in ("fit", "qstart"):
            raise ValueError(f"start is 'fit' or 'qstart', not {start!r}")
        if not self._device_model():
            raise TypeError("sample_mala integrates the model on the device: `model` must be this package's RateStateModel")
        self._ageing_only("sample_mala")
        data = np.ascontiguousarray(self.data, dtype=np.float64).reshape(-1)
        lo, hi = self.qstart_limits[:, 0], self.qstart_limits[:, 1]
        q0 = np.asarray(self.qstart, dtype=np.float64).reshape(self.n_params)
        extra = {}
        if start == "fit":
            fit = self.fit(seed=seed, device=device)
            q0 = fit.q[fit.best()]
            extra["fit"] = fit
        with Engine(mem=mem, device=device) as eng:
            eng.set_model(self.model, getattr(self.model, "substeps", 1))
            res = eng.mala(np.tile(q0, (n_chains, 1)), data, lo, hi, n_iter, eps=eps, lam=lam, seed=seed, offset=chain_offset,
                           keep=n_iter - nburn, thin=thin)
            std2 = res.std2(engine=eng, kept=True)
            eng.sync()
        return self._mala_pool(res, std2, nburn, extra)

    @staticmethod
    def _ensemble_pool(res, std2, nburn, extra=None):
        """Engine.ensemble's result and the kept states' sigma^2 → the PosteriorPool of sample_ensemble (superchains: the islands)"""
        n = res.accepted.shape[0]
        stats = {"accepted": int(res.accepted.sum()), "out_of_bounds": int(res.outbox.sum()), "stuck": int(res.stuck.sum()),
                 "evaluated": int(res.n_iter * n - res.outbox.sum() - res.stuck.sum()), "n_iter": res.n_iter, "shape": res.shape,
                 "l": res.trace_l, "n_walkers": n, "island_size": res.island_size, "n_islands": n // res.island_size, "logmask": res.logmask, "a": res.a}
        stats.update(extra or {})
        return PosteriorPool(res.trace_q, std2, res.accept_rate, stats, nburn, superchain_size=res.island_size)

    @staticmethod
    def _ensemble_mask(log_coords, d):
        return (True, True, False)[:d] if log_coords is None and d == 3 else ((False,) * d if log_coords is None else log_coords)

    @staticmethod
    def _ensemble_ball(center, lo, hi, mask, n, rng, scale=1e-3):
        """n points around `center` from N(0, scale^2) in the sampler's coordinates (log q_p under a mask bit), redrawn until inside the box"""
        center, out, todo = np.asarray(center, dtype=np.float64), np.empty((n, len(center))), np.arange(n)
        logp = np.array([(mask >> p) & 1 for p in range(len(center))], dtype=bool)
        phi = np.where(logp, np.log(np.where(logp, center, 1.0)), center)
        for _ in range(1000):
            u = phi + scale * rng.standard_normal((todo.size, len(center)))
            out[todo] = np.where(logp, np.exp(np.where(logp, u, 0.0)), u)
            todo = todo[~((out[todo] > lo) & (out[todo] < hi)).all(axis=1)]
            if todo.size == 0:
                return out
        raise ValueError("no start inside the box around the fit's point: it lies on the box's edge")

    def sample_ensemble(self, n_walkers, n_iter, nburn=None, start="fit", log_coords=None, a=2.0, seed=0, mem="device", device=-1, offset=0, thin=1,
                        iters_per_launch=16):
        """The affine-invariant ensemble sampler in islands (additive; Engine.ensemble): walkers that take their proposals from
        each other's positions (the stretch move) — no proposal covariance, no gradient, one forward solve per proposal.  An island
        is an independent ensemble of Engine.island_size walkers; n_walkers is ROUNDED UP to whole islands and the pool's
        stats["n_walkers"] reports the number run.  log_coords: per parameter, whether it moves as its logarithm; by default
        (True, True, False) with three parameters — in (log Dc, log a, b) the ridge Dc a = const is a straight line — and (False,)
        with one.  start="fit": the walkers start in a ball around self.fit(seed=seed).best()'s point, N(0, (1e-3)^2) in the
        sampler's coordinates, redrawn until inside the box; start="smc": at the final particles of Engine.smc; an array
        (n_walkers rounded, d): there.  The target is the n0 = 0 posterior pi(q) ~ 1_box SSq^-N/2, sigma^2 drawn afterwards from
        its conditional.  nburn: iterations dropped, by default n_iter // 2; every thin-th of the others is kept.  Returns a
        PosteriorPool (samples (n_keep, n_walkers, d), std2, accept_rate) whose superchains are the islands:
        pool.diagnostics() gives the nested R-hat over islands."""
        n_walkers, n_iter = int(n_walkers), int(n_iter)
        nburn = n_iter // 2 if nburn is None else int(nburn)
        if n_walkers < 1 or n_iter < 1 or not 0 <= nburn < n_iter or int(thin) < 1:
            raise ValueError("n_walkers >= 1, n_iter >= 1, 0 <= nburn < n_iter, thin >= 1")
        if isinstance(start, str) and start not in ("fit", "smc"):
            raise ValueError(f"start is 'fit', 'smc' or an array of walkers, not {start!r}")
        if not self._device_model():
            raise TypeError("sample_ensemble integrates the model on the device: `model` must be this package's RateStateModel")
        self._ageing_only("sample_ensemble")
        data = np.ascontiguousarray(self.data, dtype=np.float64).reshape(-1)
        lo, hi = self.qstart_limits[:, 0], self.qstart_limits[:, 1]
        d, extra = self.n_params, {}
        with Engine(mem=mem, device=device) as eng:
            n = whole_islands(n_walkers, eng.island_size)
            mask = eng._ens_mask(self._ensemble_mask(log_coords, d), d)
            eng.set_model(self.model, getattr(self.model, "substeps", 1))
            if isinstance(start, str) and start == "fit":
                fit = self.fit(seed=seed, device=device)
                extra["fit"] = fit
                q0 = self._ensemble_ball(fit.q[fit.best()], lo, hi, mask, n, np.random.default_rng([int(seed), int(offset)]))
            elif isinstance(start, str):
                res0 = eng.smc(data, lo, hi, n, seed=seed, offset=offset)
                q0, extra["smc_stages"] = _host(res0["q"]), len(res0["stages"])
            else:
                q0 = _host(start).reshape(-1, d)
                if q0.shape[0] != n:
                    raise ValueError(f"start holds {q0.shape[0]} walkers: {n_walkers} rounded up to whole islands of {eng.island_size} is {n}")
            res = eng.ensemble(q0, data, lo, hi, n_iter, a=a, log_coords=mask, seed=seed, offset=offset, iters_per_launch=iters_per_launch,
                               keep=n_iter - nburn, thin=thin)
            std2 = res.std2(engine=eng, kept=True)
            eng.sync()
        return self._ensemble_pool(res, std2, nburn, extra)

    @staticmethod
    def _dr_pool(res, std2, nburn, extra=None):
        """Engine.dr's result and the kept states' sigma^2 → the PosteriorPool of sample_dr"""
        n = res.q.shape[0]
        first, second = res.accept_rates
        stats = {"accepted": int(res.accepted1.sum() + res.accepted2.sum()), "accepted1": int(res.accepted1.sum()), "accepted2": int(res.accepted2.sum()),
                 "out_of_bounds": int(res.outbox1.sum()), "out_of_bounds2": int(res.outbox2.sum()), "stuck": int(res.stuck.sum()),
                 "accept_rate1": first, "accept_rate2": second, "n_solves": res.n_solves, "n_iter": res.n_iter, "shape": res.shape, "l": res.trace_l,
                 "n_chains": n, "gamma": res.gamma, "stages": res.stages, "chol": res.chol}
        stats.update(extra or {})
        return PosteriorPool(res.trace_q, std2, res.accept_rate, stats, nburn)

    def _dr_init_factor(self, eng, q0):
        """the lower Cholesky factor of the init kernel's proposal covariance at the point q0 (d,): what sample_batched proposes from"""
        self._init_chains(eng, np.asarray(q0, dtype=np.float64).reshape(1, -1), adapt_mode="none")
        V = _host(eng.get_state()[3]).reshape(self.n_params, self.n_params)
        return np.linalg.cholesky(V)

    def sample_dr(self, n_chains, n_iter, nburn=None, start="qstart", factor="init", gamma=0.2, stages=2, adapt=None, seed=0, mem="device", device=-1,
                  chain_offset=0, thin=1, iters_per_launch=16):
        """Two-stage delayed-rejection Metropolis (additive; Engine.dr): n_chains random-walk chains that, when their proposal
        q + L z is rejected — outside the box it is, without a forward solve — propose q + gamma L z' in the same iteration, with
        the correction that keeps the target exact.  No gradient, no fit and no other chain is needed.  start="qstart": every
        chain at qstart; "fit": at self.fit(seed=seed).best()'s point; an array (n_chains, d): there.  factor="init": the init
        kernel's covariance at the start point (chain 0's for an array), which sample_batched proposes from; "fit":
        FitResult.covariance(); an array (d, d): that lower triangular factor.  adapt=True: during burn-in, after every launch, L
        becomes chol(2.38^2 / d cov + eps) of every burn-in state so far, pooled over the chains (Engine.dr's adapt_launches); it is
        frozen for the kept iterations: the nburn // iters_per_launch launches that lie wholly inside the burn-in adapt.  The target is the n0 = 0 posterior
        pi(q) ~ 1_box SSq^-N/2, sigma^2 drawn afterwards from its conditional at each kept state's own Philox iteration.  A model with
        state_law="slip" runs the split path (Engine.dr_from_ssq on Engine.law_forward's sums of squares): factor is then a (d, d)
        array, start 'qstart' or an array, and nothing adapts: adapt=True raises there; a model whose observable is not 'acc' runs
        that path under either law (Engine.law_observe's sums); sample_law runs such models on the fused kernel, adapting.  adapt=None (the default) is True on the fused path and False on the split one; the pool's stats["adapt"] says which ran.  nburn:
        iterations dropped, by default n_iter // 2; every thin-th of the others is kept.  Returns a PosteriorPool; its stats carry
        both stages' acceptance (accepted1, accepted2, accept_rate1, accept_rate2), both out-of-box counts (out_of_bounds,
        out_of_bounds2), stuck, n_solves — the forward solves spent — and the factor in use at the end (chol)."""
        n_chains, n_iter, ipl = int(n_chains), int(n_iter), int(iters_per_launch)
        nburn = n_iter // 2 if nburn is None else int(nburn)
        if n_chains < 1 or n_iter < 1 or not 0 <= nburn < n_iter or int(thin) < 1 or ipl < 1:
            raise ValueError("n_chains >= 1, n_iter >= 1, 0 <= nburn < n_iter, thin >= 1, iters_per_launch >= 1")
        if isinstance(start, str) and start not in ("qstart", "fit"):
            raise ValueError(f"start is 'qstart', 'fit' or an array of chains, not {start!r}")
        if isinstance(factor, str) and factor not in ("init", "fit"):
            raise ValueError(f"factor is 'init', 'fit' or a (d, d) array, not {factor!r}")
        if not self._device_model():
            raise TypeError("sample_dr integrates the model on the device: `model` must be this package's RateStateModel")
        data = np.ascontiguousarray(self.data, dtype=np.float64).reshape(-1)
        lo, hi = self.qstart_limits[:, 0], self.qstart_limits[:, 1]
        d, extra = self.n_params, {}
        slip = self._split()  # "state_law='slip'", "observable='...'" or None
        if slip and adapt:
            raise NotImplementedError(f"sample_dr(adapt=True) under {slip}: the split path (Engine.dr_from_ssq) does not adapt the "
                                      "factor; pass adapt=False or leave it out")
        adapt = (not slip) if adapt is None else bool(adapt)
        extra["adapt"] = adapt
        if slip and (isinstance(factor, str) or (isinstance(start, str) and start == "fit")):
            raise NotImplementedError(f"sample_dr under {slip} takes factor as a (d, d) array and start 'qstart' or an array: the init "
                                      "kernel and the fit integrate the ageing law on acceleration data")
        fit = self.fit(seed=seed, device=device) if "fit" in (start if isinstance(start, str) else "", factor if isinstance(factor, str) else "") else None
        if fit is not None:
            extra["fit"] = fit
        if isinstance(start, str):
            q0 = np.tile((fit.q[fit.best()] if start == "fit" else np.asarray(self.qstart, dtype=np.float64)).reshape(1, d), (n_chains, 1))
        else:
            q0 = _host(start).reshape(-1, d)
            if q0.shape[0] != n_chains:
                raise ValueError(f"start holds {q0.shape[0]} chains, not {n_chains}")
        with Engine(mem=mem, device=device) as eng:
            eng.set_model(self.model, getattr(self.model, "substeps", 1))
            if isinstance(factor, str):
                L = self._dr_init_factor(eng, q0[0]) if factor == "init" else np.linalg.cholesky(fit.covariance())
            else:
                L = np.asarray(factor, dtype=np.float64).reshape(d, d)
            if slip:  # the split path on the plain solve's SSq; the factor stays as given (no adaptation)
                res = eng.dr_from_ssq(self._ssq_fn(eng, data), q0, lo, hi, L, n_iter, 0.5 * eng.nout, gamma=gamma, stages=stages, seed=seed,
                                      offset=chain_offset, keep=n_iter - nburn, thin=thin)
                std2 = res.std2(engine=eng, kept=True)
                eng.sync()
                return self._dr_pool(res, std2, nburn, extra)
            res = eng.dr(q0, data, lo, hi, L, n_iter, gamma=gamma, stages=stages, seed=seed, offset=chain_offset, iters_per_launch=ipl,
                         keep=n_iter - nburn, thin=thin, adapt_launches=nburn // ipl if adapt else 0)
            std2 = res.std2(engine=eng, kept=True)
            eng.sync()
        return self._dr_pool(res, std2, nburn, extra)

    def sample_law(self, n_chains, n_iter, nburn=None, start="qstart", factor="gn", gamma=0.2, stages=2, adapt=True, seed=0, mem="device", device=-1,
                   chain_offset=0, thin=1, iters_per_launch=16):
        """sample_dr's sampler on the fused kernel of the state-law solve (additive; Engine.law_dr, include/rsf_law_dr.h): for ANY
        device model — state_law "aging" or "slip", observable "acc", "mu", "theta" or "velocity", the built-in or a custom loading
        history, d = 1 or 3 — every iteration runs inside the launch, and the factor adapts.  start="qstart": every chain at
        qstart; an array (n_chains, d): there.  factor="gn": Engine.law_gn_factor at the start point (chain 0's for an array), the
        Gauss-Newton proposal from one solve of 1 + d lanes, which needs no init kernel and no fit; an array (d, d): that lower
        triangular factor.  adapt=True: the nburn // iters_per_launch launches that lie wholly inside the burn-in adapt the factor
        (Engine.dr's adapt_launches), then it is frozen.  Everything else — the target, sigma^2, nburn, thin, the returned
        PosteriorPool and its stats — is sample_dr's; stats["adapt"] says whether the factor adapted and stats["path"] is "law_dr"."""
        n_chains, n_iter, ipl = int(n_chains), int(n_iter), int(iters_per_launch)
        nburn = n_iter // 2 if nburn is None else int(nburn)
        if n_chains < 1 or n_iter < 1 or not 0 <= nburn < n_iter or int(thin) < 1 or ipl < 1:
            raise ValueError("n_chains >= 1, n_iter >= 1, 0 <= nburn < n_iter, thin >= 1, iters_per_launch >= 1")
        if isinstance(start, str) and start != "qstart":
            raise ValueError(f"start is 'qstart' or an array of chains, not {start!r}")
        if isinstance(factor, str) and factor != "gn":
            raise ValueError(f"factor is 'gn' or a (d, d) array, not {factor!r}")
        if not self._device_model():
            raise TypeError("sample_law integrates the model on the device: `model` must be this package's RateStateModel")
        data = np.ascontiguousarray(self.data, dtype=np.float64).reshape(-1)
        lo, hi = self.qstart_limits[:, 0], self.qstart_limits[:, 1]
        d, law, observable = self.n_params, self._law(), self._observable()
        if isinstance(start, str):
            q0 = np.tile(np.asarray(self.qstart, dtype=np.float64).reshape(1, d), (n_chains, 1))
        else:
            q0 = _host(start).reshape(-1, d)
            if q0.shape[0] != n_chains:
                raise ValueError(f"start holds {q0.shape[0]} chains, not {n_chains}")
        with Engine(mem=mem, device=device) as eng:
            eng.set_model(self.model, getattr(self.model, "substeps", 1))
            L = eng.law_gn_factor(law, observable, q0[0], data)[0] if isinstance(factor, str) else np.asarray(factor, dtype=np.float64).reshape(d, d)
            res = eng.law_dr(law, observable, q0, data, lo, hi, L, n_iter, gamma=gamma, stages=stages, seed=seed, offset=chain_offset,
                             iters_per_launch=ipl, keep=n_iter - nburn, thin=thin, adapt_launches=nburn // ipl if adapt else 0)
            std2 = res.std2(engine=eng, kept=True)
            eng.sync()
        return self._dr_pool(res, std2, nburn, {"adapt": bool(adapt), "path": "law_dr"})

    def sample_stiffness(self, n_chains, n_iter, stiffness_prior, nburn=None, start="qstart", factor="gn", gamma=0.2, stages=2, adapt=True, seed=0,
                         mem="device", device=-1, chain_offset=0, thin=1, iters_per_launch=16):
        """sample_law with the STIFFNESS OF THE APPARATUS INFERRED jointly (additive; Engine.kstiff_dr, include/rsf_kstiff.h): the
        chains run over (Dc, k) for a one-parameter MCMC and over (Dc, a, b, k) for a three-parameter one, the stiffness the LAST
        parameter of the returned PosteriorPool, under a uniform prior stiffness_prior = (klo, khi) with
        0 < klo < model.stiffness < khi.  model.stiffness, the calibration's value, is where the chains start and nothing more:
        start="qstart" puts every chain at (qstart..., model.stiffness); an array (n_chains, d + 1): there.  factor="gn":
        Engine.kstiff_gn_factor at the start point (chain 0's for an array); an array (d + 1, d + 1): that lower triangular factor.
        Everything else — the sampler, adapt, the target, sigma^2, nburn, thin, the PosteriorPool and its stats — is sample_law's;
        stats["path"] is "kstiff_dr".  The MCMC object itself stays d = 1 or 3.

        Why: a stiffness from a calibration run is good to some 10-20 %, and a wrong fixed value moves Dc.  On friction data from
        Dc = 20, k = 2e-3 (noise 5 %, 500 steps) k fixed 20 % off puts the best Dc at 19.0 or 21.0 under a velocity-step history
        and at 16.75 or 24.5 under a hold history: an 18 % error.

        WHAT THE DATA DETERMINE depends on the loading history.  Under a velocity-step history all of (Dc, a, b, k) are determined:
        at the truth the Gauss-Newton (Laplace) SDs are 1.2 %, 0.9 %, 0.6 % and 1.5 % of the values under the ageing law (1.6 %,
        1.1 %, 0.7 %, 1.4 % under the slip law), and the column-scaled Jacobian's condition number is 7 (8).  Under a HOLD history
        the four-parameter problem is nearly degenerate: the SDs of (Dc, a, b, k) are 101 %, 8 %, 50 % and 1.7 % of the values and
        the condition number is 160, so the d = 4 posterior there is set by the prior box as much as by the data, the Gauss-Newton
        factor is a poor start and the chains mix slowly.  That is a fact about the experiment, not the sampler.  The two-parameter
        problem (Dc, k), with (a, b) known, is well determined under both histories (SDs 0.6-1.6 %, condition number below 2).
        (tests/test_kstiff_reference.py asserts every figure here to 3 % of it.)"""
        n_chains, n_iter, ipl = int(n_chains), int(n_iter), int(iters_per_launch)
        nburn = n_iter // 2 if nburn is None else int(nburn)
        if n_chains < 1 or n_iter < 1 or not 0 <= nburn < n_iter or int(thin) < 1 or ipl < 1:
            raise ValueError("n_chains >= 1, n_iter >= 1, 0 <= nburn < n_iter, thin >= 1, iters_per_launch >= 1")
        if isinstance(start, str) and start != "qstart":
            raise ValueError(f"start is 'qstart' or an array of chains, not {start!r}")
        if isinstance(factor, str) and factor != "gn":
            raise ValueError(f"factor is 'gn' or a (d + 1, d + 1) array, not {factor!r}")
        if not self._device_model():
            raise TypeError("sample_stiffness integrates the model on the device: `model` must be this package's RateStateModel")
        k0 = self._stiffness()
        if k0 is None:
            raise ValueError("sample_stiffness starts the chains at model.stiffness, the calibration's value: the model has none")
        klo, khi = (float(v) for v in stiffness_prior)
        if not (math.isfinite(khi) and 0.0 < klo < k0 < khi):
            raise ValueError(f"stiffness_prior = (klo, khi) with 0 < klo < model.stiffness < khi, not ({klo!r}, {khi!r}) around {k0!r}")
        check_law_options(self.model)  # integrator='dop853', precision='float32': NotImplementedError, the solve is the float64 RK4
        data = np.ascontiguousarray(self.data, dtype=np.float64).reshape(-1)
        lo, hi = np.append(self.qstart_limits[:, 0], klo), np.append(self.qstart_limits[:, 1], khi)
        d, law, observable = self.n_params + 1, self._law(), self._observable()
        if isinstance(start, str):
            q0 = np.tile(np.append(np.asarray(self.qstart, dtype=np.float64).reshape(-1), k0).reshape(1, d), (n_chains, 1))
        else:
            q0 = _host(start).reshape(-1, d)
            if q0.shape[0] != n_chains:
                raise ValueError(f"start holds {q0.shape[0]} chains, not {n_chains}")
        with Engine(mem=mem, device=device) as eng:
            eng.set_model(self.model, getattr(self.model, "substeps", 1))
            L = eng.kstiff_gn_factor(law, observable, q0[0], data)[0] if isinstance(factor, str) else np.asarray(factor, dtype=np.float64).reshape(d, d)
            res = eng.kstiff_dr(law, observable, q0, data, lo, hi, L, n_iter, gamma=gamma, stages=stages, seed=seed, offset=chain_offset,
                                iters_per_launch=ipl, keep=n_iter - nburn, thin=thin, adapt_launches=nburn // ipl if adapt else 0)
            std2 = res.std2(engine=eng, kept=True)
            eng.sync()
        return self._dr_pool(res, std2, nburn, {"adapt": bool(adapt), "path": "kstiff_dr"})

    def quadrature(self, n=None, n_draws=0, seed=0, coords=None, window_sd=12.0, mem="device", device=-1):
        """The exact posterior by quadrature on the GPU (additive; Engine.grid_posterior): the n0 = 0 target
        pi(q) ~ 1_box SSq^-N/2 tabulated on a tensor grid over the prior box — d = 1: n = (4001,) Simpson nodes of Dc; d = 3:
        n = (2001, 65, 65) nodes of (Dc a, a, b), the product an axis so that the ridge Dc a = const is resolved.  Returns a
        GridPosterior: log_evidence, mean, cov, std2_mean, marginal(name), quantiles(name, probs) carry no Monte Carlo error;
        draw(n) gives independent draws and pool(n) a PosteriorPool of them on which predictive, loo, joint, corner and the
        diagnostics work unchanged.  n_draws > 0: that many draws are taken at once and kept as .q and .std2.  The result holds
        its engine (result.engine.close() releases it)."""
        if not self._device_model():
            raise TypeError("quadrature integrates the model on the device: `model` must be this package's RateStateModel")
        data = np.ascontiguousarray(self.data, dtype=np.float64).reshape(-1)
        lo, hi = self.qstart_limits[:, 0], self.qstart_limits[:, 1]
        eng = Engine(mem=mem, device=device)
        try:
            eng.set_model(self.model, getattr(self.model, "substeps", 1))
            if self._split():  # the same two stages, the nodes solved by law_forward or law_observe
                if self.n_params != 1:
                    raise NotImplementedError(f"quadrature under {self._split()} is one-parameter (Dc)")
                res = eng.grid_posterior(data, lo, hi, n=n, coords=coords, window_sd=window_sd, ssq_fn=self._ssq_fn(eng, data))
            else:
                res = eng.grid_posterior(data, lo, hi, n=n, coords=coords, window_sd=window_sd)
            res.q, res.std2 = res.draw(int(n_draws), seed) if int(n_draws) > 0 else (None, None)
            eng.sync()
        except BaseException:
            eng.close()
            raise
        return res

    def compare_laws(self, laws=("aging", "slip"), **quadrature_kw):
        """Ageing law or slip law?  The exact posterior of Dc under each state law by quadrature() (one parameter) and the log
        Bayes factor between them → dict with a GridPosterior per entry of `laws` (keyed as given) and log_bayes_factor, the slip
        law's log evidence minus the ageing law's.  quadrature_kw: quadrature's arguments.  The model's state_law is restored
        afterwards.  Under the reference's built-in loading history the slider stays at steady state and the two laws give the
        same series (log Bayes factor 0): the laws separate under a velocity-step or slide-hold-slide history (model.loading)."""
        if self._multi_parameter():
            raise NotImplementedError("compare_laws is one-parameter (Dc)")
        if sorted(law_name(law) for law in laws) != ["aging", "slip"]:
            raise ValueError(f"laws names the ageing and the slip law once each, not {laws!r}")
        before, out, ev = getattr(self.model, "state_law", "aging"), {}, {}
        try:
            for law in laws:
                self.model.state_law = law
                out[law] = self.quadrature(**quadrature_kw)
                ev[self._law()] = out[law].log_evidence
        finally:
            self.model.state_law = before
        out["log_bayes_factor"] = ev["slip"] - ev["aging"]
        return out

    def quadrature_law(self, n=None, n_starts=64, window_sd=8.0, log_coords=None, marginals=("Dc",), n_draws=0, seed=0, mem="device", device=-1):
        """The exact posterior by quadrature for ANY device model at d = 1 or 3 (additive; Engine.law_grid_posterior,
        include/rsf_law_grid.h): state_law "aging" or "slip", observable "acc", "mu", "theta" or "velocity", the built-in or a custom
        loading history.  fit_law from n_starts starts gives the point (FitResult.best()) and its covariance; the tensor grid is laid
        in the whitened coordinates of that fit, n (default 65 per axis) Simpson nodes on +- window_sd per axis, log_coords naming
        the parameters whose logarithm is the working coordinate (on acceleration data ("Dc", "a") straightens the ridge).  One grid
        per name in `marginals`, with that parameter on axis 0: each extra name costs one more grid.  → the first grid's
        LawGridPosterior (log_evidence, mean, cov, std2_mean, marginal(), quantiles(probs), cdf(xs), draw(n), pool(n), edge_mass,
        n_neginf, n_solves) with .grids {name: LawGridPosterior}, .evidence_spread (the largest minus the smallest log_evidence over
        the grids: what the order of the axes changes), .fit (the FitResult) and, with n_draws > 0, .q and .std2.  The result holds
        its engine (result.engine.close() releases it)."""
        if not self._device_model():
            raise TypeError("quadrature_law integrates the model on the device: `model` must be this package's RateStateModel")
        self._coupled_only("quadrature_law (and bayes_factor_laws)")
        names = ("Dc", "a", "b")[:self.n_params]
        marginals = (marginals,) if isinstance(marginals, str) else tuple(marginals)
        if not marginals or any(k not in names for k in marginals) or len(set(marginals)) != len(marginals):
            raise ValueError(f"marginals names parameters of {names}, each once, at least one")
        data = np.ascontiguousarray(self.data, dtype=np.float64).reshape(-1)
        lo, hi = self.qstart_limits[:, 0], self.qstart_limits[:, 1]
        d, law, observable = self.n_params, self._law(), self._observable()
        eng = Engine(mem=mem, device=device)
        try:
            eng.set_model(self.model, getattr(self.model, "substeps", 1))
            q0, _, _ = self._fit_starts(eng, n_starts, seed)
            fit = eng.law_fit(law, observable, q0, data, lo, hi)
            i = fit.best()
            point, cov = fit.q[i].copy(), fit.covariance(i)
            logged = [names.index(k) if isinstance(k, str) and k in names else int(k) for k in (log_coords or ())]
            J = np.ones(d)
            J[logged] = 1.0 / point[logged]
            try:
                F = np.linalg.cholesky(cov * J[:, None] * J[None, :])
            except np.linalg.LinAlgError:
                raise RsfError(ERR_NOT_POSDEF, "quadrature_law: the fit's covariance is not positive definite (a fit on a face of the box?)") from None
            grids = {k: eng.law_grid_posterior(law, observable, data, lo, hi, point, F, log_coords=logged, first=k, n=n, window_sd=window_sd)
                     for k in marginals}
            res = grids[marginals[0]]
            ev = [g.log_evidence for g in grids.values()]
            res.grids, res.evidence_spread, res.fit = grids, float(max(ev) - min(ev)), fit
            res.q, res.std2 = res.draw(int(n_draws), seed) if int(n_draws) > 0 else (None, None)
            eng.sync()
        except BaseException:
            eng.close()
            raise
        return res

    def bayes_factor_laws(self, laws=("aging", "slip"), **quadrature_kw):
        """compare_laws at d = 1 or 3 on quadrature_law: the exact posterior under each state law and the log Bayes factor between
        them → dict with a LawGridPosterior per entry of `laws` (keyed as given) and log_bayes_factor, the slip law's log evidence
        minus the ageing law's.  quadrature_kw: quadrature_law's arguments.  The model's state_law is restored afterwards.  Each
        result holds its engine (out[law].engine.close() releases it); if a law's quadrature raises, the engines of the laws
        already done are closed here.  A law
        that the data contradict is often fitted onto a face of the box: its grid then has n_neginf > 0 and its evidence is
        approximate — by far less than such a Bayes factor is large."""
        if sorted(law_name(law) for law in laws) != ["aging", "slip"]:
            raise ValueError(f"laws names the ageing and the slip law once each, not {laws!r}")
        before, out, ev = getattr(self.model, "state_law", "aging"), {}, {}
        try:
            for law in laws:
                self.model.state_law = law
                out[law] = self.quadrature_law(**quadrature_kw)
                ev[self._law()] = out[law].log_evidence
        except BaseException:
            for res in out.values():  # the engines of the laws already done: nobody else holds them
                res.engine.close()
            raise
        finally:
            self.model.state_law = before
        out["log_bayes_factor"] = ev["slip"] - ev["aging"]
        return out

    def _fit_starts(self, eng, n_starts, seed):
        """start 0 is qstart, the others rsf_smc_init's uniform start in the prior box (seed, particles 0 .. n_starts - 2)"""
        lo, hi = self.qstart_limits[:, 0], self.qstart_limits[:, 1]
        q0 = np.asarray(self.qstart, dtype=np.float64).reshape(1, self.n_params)
        if int(n_starts) < 1:
            raise ValueError("n_starts must be >= 1")
        if int(n_starts) > 1:
            q0 = np.concatenate([q0, _host(eng.smc_init(lo, hi, int(n_starts) - 1, seed))])
        return q0, lo, hi

    def fit(self, n_starts=64, seed=0, mem="host", device=-1, **kw):
        """Least squares before any sampling (additive; Engine.fit): a Levenberg-Marquardt fit from n_starts start points at once —
        start 0 is qstart, the others are uniform in the prior box — each iteration one group solve on the GPU.  Returns a
        FitResult: best() is the start with the smallest sum of squares, covariance() its least-squares covariance, laplace() a
        quick evidence to set beside PosteriorPool.evidence and sample_smc's.  sample_batched(q0=...) takes best()'s point as the
        chains' start.  With three parameters the estimate is ONE POINT on the ridge Dc a = const: only its sum of squares and
        Dc a are reproducible.  kw: Engine.fit's fd_rel_step, ftol, max_iter, iters_per_launch."""
        if not self._device_model():
            raise TypeError("fit integrates the model on the device: `model` must be this package's RateStateModel")
        self._ageing_only("fit")
        data = np.ascontiguousarray(self.data, dtype=np.float64).reshape(-1)
        with Engine(mem=mem, device=device) as eng:
            eng.set_model(self.model, getattr(self.model, "substeps", 1))
            q0, lo, hi = self._fit_starts(eng, n_starts, seed)
            res = eng.fit(q0, data, lo, hi, **kw)
            eng.sync()
            return res

    def fit_law(self, n_starts=64, seed=0, mem="host", device=-1, **kw):
        """fit on the kernels of the state-law solve (additive; Engine.law_fit, include/rsf_law_fit.h): for ANY device model —
        state_law "aging" or "slip", observable "acc", "mu", "theta" or "velocity", the built-in or a custom loading history,
        d = 1 or 3 — the Levenberg-Marquardt fit from fit's start points (qstart, then uniform in the prior box), every iteration
        inside the launch.  Returns fit's FitResult; best()'s point is a start for sample_law (start=np.tile(point, (n_chains, 1)))
        from which its factor="gn" has a Cholesky factor.  kw: Engine.law_fit's fd_rel_step, ftol, max_iter, iters_per_launch.
        A model with a stiffness (model.stiffness) runs Engine.fit_from_residuals around Engine.law_observe instead: the fused
        kernel integrates k' = 0.1 / Dc."""
        if not self._device_model():
            raise TypeError("fit_law integrates the model on the device: `model` must be this package's RateStateModel")
        data = np.ascontiguousarray(self.data, dtype=np.float64).reshape(-1)
        with Engine(mem=mem, device=device) as eng:
            eng.set_model(self.model, getattr(self.model, "substeps", 1))
            q0, lo, hi = self._fit_starts(eng, n_starts, seed)
            if self._stiffness() is not None:  # the split route: the GPU's trial points and decisions around law_observe's series
                kw.pop("iters_per_launch", None)
                law, observable = self._law(), self._observable()

                def residuals(pts):
                    ab = [np.ascontiguousarray(pts[:, p]) for p in (1, 2)] if pts.shape[1] == 3 else [None, None]
                    series = _host(eng.law_observe(law, observable, np.ascontiguousarray(pts[:, 0]), ab[0], ab[1])[1])
                    return series.T - data[None, :]

                res = eng.fit_from_residuals(residuals, q0, lo, hi, **kw)
                eng.sync()
                return res
            res = eng.law_fit(self._law(), self._observable(), q0, data, lo, hi, **kw)
            eng.sync()
            return res

    # ---- visualisation (off the hot path; degrades gracefully) --------------------------
    def _animate(self, qparams):
        _figures.chain_movie(qparams[0], f"MCMC Sampling Evolution for dc = {self.dc_true:.2f} as True value",
                             f"mcmc_animation_dc_{self.dc_true:.2f}.mp4")


assert set(ADAPT_MODES) == {"none", "reference_dict", "am"}
