"""
RSF — drop-in for the reference driver class (RSF.py:59-1046): sweeps `dc_list`, makes the
synthetic observation, round-trips it through the chosen persistence format and runs one
MCMC per Dc.  The compute (forward solves, sampling) goes to the GPU; plotting stays optional
host work and never blocks the result.

Deviations from the reference, all needed for `main.py` to run at all:
the JSON helpers are imported under their own names (the reference shadows them with the MySQL
ones), the MySQL helpers are imported lazily, and a missing ffmpeg/display only skips figures.
"""
import time

import numpy as np

if __package__:
    from . import _figures, json_save_load
    from .engine import DrResult, Engine, EnsembleResult, MalaResult, whole_islands
    from .MCMC import MCMC, PosteriorPool
else:  # flat layout: this directory on sys.path, the reference's own import style (main.py:44-46)
    import _figures
    import json_save_load
    from engine import DrResult, Engine, EnsembleResult, MalaResult, whole_islands
    from MCMC import MCMC, PosteriorPool


def measure_execution_time(func):
    """Wall-clock decorator; like the reference (RSF.py:49-54) it RETURNS the elapsed seconds."""

    def wrapper(*args, **kwargs):
        start_time = time.time()
        func(*args, **kwargs)
        return time.time() - start_time

    return wrapper


class RSF:
    def __init__(self, number_slip_values=1, lowest_slip_value=1.0, largest_slip_value=1000.0, qstart=10.0,
                 qpriors=["Uniform", 0.0, 10000.0], reduction=False, plotfigs=False):
        self.num_dc = number_slip_values
        self.dc_list = np.linspace(lowest_slip_value, largest_slip_value, self.num_dc)
        self.num_features = 2
        self.plotfigs = plotfigs
        self.qstart = qstart
        self.qpriors = qpriors
        self.reduction = reduction
        self.make_animations = True   # the reference hard-codes sample(True), RSF.py:897
        self.verbose = True
        self.posteriors = {}          # additive: dc -> kept samples of the last inference

    def generate_time_series(self):
        """Noisy acceleration for every Dc of dc_list, concatenated (RSF.py:355-371).  The
        forward solves run as ONE batched launch; the noise is drawn per Dc in the reference's
        order from the global NumPy RNG."""
        n = self.model.num_tsteps
        acc = self.model.evaluate_batch(self.dc_list)  # (num_dc, nout)
        if acc.shape[1] != n:
            raise ValueError(f"model produces {acc.shape[1]} samples per series, num_tsteps is {n}")
        acc_appended_noise = np.zeros(len(self.dc_list) * n)
        t = self.model.time_axis()
        for index, dc_value in enumerate(self.dc_list):
            self.model.Dc = dc_value
            acc_noise = acc[index] + 1.0 * np.abs(acc[index]) * np.random.randn(n)  # RateStateModel.py:392
            self.plot_time_series(t, acc[index])
            acc_appended_noise[index * n:(index + 1) * n] = acc_noise
        return acc_appended_noise

    def plot_time_series(self, time, acceleration):
        if self.plotfigs:
            _figures.series_figure(time, acceleration, self.model.Dc, self.model.t_start, self.model.t_final)

    def prepare_data(self, data):
        if self.format == "json":
            self.lstm_file = "model_lstm.json"
            self.data_file = "data.json"
            json_save_load.save_object(data, self.data_file)
            data = json_save_load.load_object(self.data_file)
        elif self.format == "mysql":
            raise RuntimeError("the MySQL format needs a server and mysql.connector (RSF.py:597-602); "
                               "neither is part of this build — use 'json'")
        return data

    def plot_dist(self, qparams, dc):
        """Kept samples beside their kernel density (RSF.py:717-746); the density is the device KDE of the pooled draws."""
        def kde():  # resolved inside the figure's guard: an engine failure only skips the figure
            return self.model.engine().pool_kde

        kde._deferred = True
        return _figures.trace_with_density(qparams[0, :], f"$d_c={dc:.2f}\\,\\mu m$ with {self.format} formatting", kde)

    def perform_sampling_and_plotting(self, data, dc, nsamples, model_lstm):
        hits = np.flatnonzero(np.asarray(self.dc_list) == dc)  # the series of true value dc_list[i] is data[i*N:(i+1)*N], RSF.py:874-882
        if hits.size == 0:
            print(f"Error: dc value {dc} not found in dc_list.")
            return
        n = self.model.num_tsteps
        noisy_data = data[int(hits[0]) * n:(int(hits[0]) + 1) * n]
        print(f"--- Dc is {dc} ---")
        mc = MCMC(self.model, noisy_data, dc, self.qpriors, self.qstart, lstm_model=model_lstm, nsamples=nsamples,
                  verbose=self.verbose)
        qparams = mc.sample(self.make_animations)
        self.posteriors[float(dc)] = qparams
        self.plot_dist(qparams, dc)

    def inference_batched(self, nsamples, chains_per_dc=256, seed=0, mem="device", device=-1, adapt_mode=None):
        """Additive throughput path: the whole dc_list sweep as ONE launch per block of iterations — every
        true Dc is an observation group with `chains_per_dc` independent chains (Philox variates on device).
        Returns {dc: PosteriorPool} of the post-burn-in draws (nburn = int(nsamples/2) like MCMC)."""
        n, G = self.model.num_tsteps, len(self.dc_list)
        data = np.ascontiguousarray(np.asarray(self.data, dtype=np.float64).reshape(G, n))
        probe = MCMC(self.model, data[0], self.dc_list[0], self.qpriors, self.qstart, nsamples=nsamples)
        nburn = probe.nburn
        C = G * int(chains_per_dc)
        eng = Engine(mem=mem, device=device)
        try:
            eng.set_model(self.model, getattr(self.model, "substeps", 1))
            eng.mcmc_init(np.full((C, 1), float(self.qstart)), data, probe.qstart_limits[:, 0], probe.qstart_limits[:, 1],
                          seed=seed, n0=probe.n0, prior_len=len(self.qpriors), adapt_mode=adapt_mode or probe._adapt_mode(),
                          adapt_interval=probe.adapt_interval)
            tq, ts, ta = eng.mcmc_run(nsamples)
            eng.sync()
            tq, ts, ta = (np.asarray(x.cpu() if hasattr(x, "cpu") else x) for x in (tq, ts, ta))
        finally:
            eng.close()
        out, first = {}, max(nburn - 1, 0)
        for g, dc in enumerate(self.dc_list):
            sl = slice(g * chains_per_dc, (g + 1) * chains_per_dc)
            acc = int(ta[:, sl].sum())
            out[float(dc)] = PosteriorPool(tq[first:, sl], ts[first:, sl], acc / (nsamples * chains_per_dc),
                                           dict(accepted=acc), nburn)
        self.posteriors = {dc: pool.pooled() for dc, pool in out.items()}
        return out

    def inference_smc(self, n_particles, replicates=1, seed=0, mem="device", device=-1, ess_fraction=0.5, steps=3, max_stages=200):
        """Additive: tempered SMC over the whole dc_list sweep in ONE batch (Engine.smc_batch) — every true Dc is an observation
        group with `replicates` independent populations of n_particles (seeds seed .. seed + replicates - 1), no start point and
        no burn-in, so the Dc far from qstart cost no more than the others.  Returns {dc: PosteriorPool} of each group's first
        replicate (MCMC.sample_smc's pool); its stats carry replicate_log_evidence, log_evidence_mean and log_evidence_se over the
        group's replicates (se NaN for one).  The `inference` path is not touched."""
        n, G = self.model.num_tsteps, len(self.dc_list)
        data = np.ascontiguousarray(np.asarray(self.data, dtype=np.float64).reshape(G, n))
        probe = MCMC(self.model, data[0], self.dc_list[0], self.qpriors, self.qstart, nsamples=10)
        with Engine(mem=mem, device=device) as eng:
            eng.set_model(self.model, getattr(self.model, "substeps", 1))
            res = eng.smc_batch(data, probe.qstart_limits[:, 0], probe.qstart_limits[:, 1], int(n_particles), seeds=int(seed),
                                replicates=int(replicates), ess_fraction=ess_fraction, steps=steps, max_stages=max_stages)
            eng.sync()
            out = {}
            for g, (dc, summ) in enumerate(zip(self.dc_list, res["summary"])):
                runs = res["runs"][g * int(replicates):(g + 1) * int(replicates)]
                out[float(dc)] = MCMC._smc_pool(runs[0], {"replicate_log_evidence": np.array([r["log_evidence"] for r in runs]),
                                                          "log_evidence_mean": summ["log_evidence_mean"], "log_evidence_se": summ["log_evidence_se"]})
        self.posteriors = {dc: pool.pooled() for dc, pool in out.items()}
        return out

    def inference_fit(self, n_starts=64, seed=0, mem="host", device=-1, **kw):
        """Additive: the least-squares estimate of every true Dc of dc_list in ONE call (Engine.fit) — each is an observation group
        with n_starts start points (MCMC.fit's: qstart, then uniform in the prior box).  Returns {dc: dict(q, ssq, cov, stderr,
        status, iters, index)} of each group's best start; the FitResult of all starts is kept in self.fit_result.  The
        `inference` path is not touched."""
        n, G = self.model.num_tsteps, len(self.dc_list)
        data = np.ascontiguousarray(np.asarray(self.data, dtype=np.float64).reshape(G, n))
        probe = MCMC(self.model, data[0], self.dc_list[0], self.qpriors, self.qstart, nsamples=10)
        with Engine(mem=mem, device=device) as eng:
            eng.set_model(self.model, getattr(self.model, "substeps", 1))
            q0, lo, hi = probe._fit_starts(eng, n_starts, seed)
            res = eng.fit(np.tile(q0, (G, 1)), data, lo, hi, **kw)
            eng.sync()
        self.fit_result, out = res, {}
        for g, dc in enumerate(self.dc_list):
            i = res.best(g)
            cov = res.covariance(i)
            out[float(dc)] = {"q": res.q[i].copy(), "ssq": float(res.ssq[i]), "cov": cov, "stderr": np.sqrt(np.diag(cov)),
                              "status": int(res.status[i]), "iters": int(res.iters[i]), "index": i}
        return out

    def inference_mala(self, n_chains=256, n_iter=200, nburn=None, start="fit", seed=0, eps=1.0, lam=1e-3, mem="device", device=-1, thin=1):
        """Additive: the posterior of every true Dc of dc_list by Gauss-Newton manifold MALA in ONE call (Engine.mala) — each is
        an observation group of n_chains chains, started at its group's least-squares estimate (start="fit": inference_fit) or at
        qstart (start="qstart").  Returns {dc: PosteriorPool} as MCMC.sample_mala gives it for one group; chain j of group g draws
        from the Philox stream (seed, g * (n_chains padded to whole workgroups) + j).  The `inference` path is not touched."""
        n_chains, n_iter = int(n_chains), int(n_iter)
        nburn = n_iter // 2 if nburn is None else int(nburn)
        if n_chains < 1 or n_iter < 1 or not 0 <= nburn < n_iter or int(thin) < 1:
            raise ValueError("n_chains >= 1, n_iter >= 1, 0 <= nburn < n_iter, thin >= 1")
        if start not in ("fit", "qstart"):
            raise ValueError(f"start is 'fit' or 'qstart', not {start!r}")
        n, G = self.model.num_tsteps, len(self.dc_list)
        data = np.ascontiguousarray(np.asarray(self.data, dtype=np.float64).reshape(G, n))
        probe = MCMC(self.model, data[0], self.dc_list[0], self.qpriors, self.qstart, nsamples=10)
        lo, hi = probe.qstart_limits[:, 0], probe.qstart_limits[:, 1]
        starts = np.tile(np.asarray(self.qstart, dtype=np.float64).reshape(1, probe.n_params), (G, 1))
        if start == "fit":
            est = self.inference_fit(seed=seed, mem=mem, device=device)
            starts = np.stack([est[float(dc)]["q"] for dc in self.dc_list])
        out = {}
        with Engine(mem=mem, device=device) as eng:
            eng.set_model(self.model, getattr(self.model, "substeps", 1))
            res = eng.mala(np.repeat(starts, n_chains, axis=0), data, lo, hi, n_iter, eps=eps, lam=lam, seed=seed, keep=n_iter - nburn, thin=thin)
            std2 = res.std2(engine=eng, kept=True)
            eng.sync()
        self.mala_result = res
        for g, dc in enumerate(self.dc_list):
            s = slice(g * n_chains, (g + 1) * n_chains)
            part = MalaResult(res.q[s], res.ssq[s], res.grad[s], res.jtj[s], res.accepted[s], res.outbox[s], res.stuck[s], res.n_iter,
                              res.samples[:, s], res.ssq_trace[:, s], res.iterations, res.shape, res.seed, res.offset)
            out[float(dc)] = MCMC._mala_pool(part, std2[:, s], nburn)
        return out

    def inference_grid(self, n=None, n_draws=0, seed=0, coords=None, window_sd=12.0, mem="device", device=-1):
        """Additive: the exact posterior of every true Dc of dc_list by quadrature on the GPU (MCMC.quadrature, one grid per
        observation group).  Returns {dc: GridPosterior}; with n_draws > 0 each carries that many independent draws (.q, .std2),
        group g from the Philox stream (seed, g * n_draws + j).  ALL the results hold ONE engine, self.grid_engine: draw, pool and
        marginal('Dc') of every one of them need it open, so close it (self.grid_engine.close(), the same object as any
        result's .engine) only when done with all of them.  An error closes it.  The `inference` path is not touched."""
        nt, G = self.model.num_tsteps, len(self.dc_list)
        data = np.ascontiguousarray(np.asarray(self.data, dtype=np.float64).reshape(G, nt))
        probe = MCMC(self.model, data[0], self.dc_list[0], self.qpriors, self.qstart, nsamples=10)
        lo, hi = probe.qstart_limits[:, 0], probe.qstart_limits[:, 1]
        out = {}
        eng = Engine(mem=mem, device=device)
        try:
            eng.set_model(self.model, getattr(self.model, "substeps", 1))
            for g, dc in enumerate(self.dc_list):
                res = eng.grid_posterior(data[g], lo, hi, n=n, coords=coords, window_sd=window_sd)
                res.q, res.std2 = res.draw(int(n_draws), seed, g * int(n_draws)) if int(n_draws) > 0 else (None, None)
                out[float(dc)] = res
            eng.sync()
        except BaseException:
            eng.close()
            raise
        self.grid_engine, self.grid_result = eng, out
        return out

    def inference_ensemble(self, n_walkers=512, n_iter=200, nburn=None, start="fit", log_coords=None, a=2.0, seed=0, mem="device", device=-1, thin=1):
        """Additive: the posterior of every true Dc of dc_list by the affine-invariant ensemble sampler in ONE call
        (Engine.ensemble) — each is an observation group of n_walkers walkers (rounded up to whole islands), started in a ball
        around its group's least-squares estimate (start="fit": inference_fit) or around qstart (start="qstart").  Returns
        {dc: PosteriorPool} as MCMC.sample_ensemble gives it for one group; walker j of group g draws from the Philox stream
        (seed, g * n_walkers + j).  The `inference` path is not touched."""
        n_walkers, n_iter = int(n_walkers), int(n_iter)
        nburn = n_iter // 2 if nburn is None else int(nburn)
        if n_walkers < 1 or n_iter < 1 or not 0 <= nburn < n_iter or int(thin) < 1:
            raise ValueError("n_walkers >= 1, n_iter >= 1, 0 <= nburn < n_iter, thin >= 1")
        if start not in ("fit", "qstart"):
            raise ValueError(f"start is 'fit' or 'qstart', not {start!r}")
        n, G = self.model.num_tsteps, len(self.dc_list)
        data = np.ascontiguousarray(np.asarray(self.data, dtype=np.float64).reshape(G, n))
        probe = MCMC(self.model, data[0], self.dc_list[0], self.qpriors, self.qstart, nsamples=10)
        lo, hi = probe.qstart_limits[:, 0], probe.qstart_limits[:, 1]
        d = probe.n_params
        starts = np.tile(np.asarray(self.qstart, dtype=np.float64).reshape(1, d), (G, 1))
        if start == "fit":
            est = self.inference_fit(seed=seed, mem=mem, device=device)
            starts = np.stack([est[float(dc)]["q"] for dc in self.dc_list])
        out = {}
        with Engine(mem=mem, device=device) as eng:
            per = whole_islands(n_walkers, eng.island_size)
            mask = eng._ens_mask(MCMC._ensemble_mask(log_coords, d), d)
            eng.set_model(self.model, getattr(self.model, "substeps", 1))
            q0 = np.concatenate([MCMC._ensemble_ball(starts[g], lo, hi, mask, per, np.random.default_rng([int(seed), g])) for g in range(G)])
            res = eng.ensemble(q0, data, lo, hi, n_iter, a=a, log_coords=mask, seed=seed, keep=n_iter - nburn, thin=thin)
            std2 = res.std2(engine=eng, kept=True)
            eng.sync()
        self.ensemble_result = res
        for g, dc in enumerate(self.dc_list):
            s = slice(g * per, (g + 1) * per)
            part = EnsembleResult(res.q[s], res.l[s], res.accepted[s], res.outbox[s], res.stuck[s], res.n_iter, res.trace_q[:, s], res.trace_l[:, s],
                                  res.iterations, res.island_size, res.shape, res.seed, res.offset + g * per, res.logmask, res.a)
            out[float(dc)] = MCMC._ensemble_pool(part, std2[:, s], nburn)
        return out

    def inference_dr(self, n_chains=256, n_iter=200, nburn=None, start="qstart", factor="init", gamma=0.2, stages=2, adapt=True, seed=0, mem="device",
                     device=-1, thin=1, iters_per_launch=16):
        """Additive: the posterior of every true Dc of dc_list by two-stage delayed-rejection Metropolis in ONE call (Engine.dr) —
        each is an observation group of n_chains chains (rounded up to whole workgroups when there is more than one group) with
        its own proposal factor, started at qstart (start="qstart") or at its group's least-squares estimate (start="fit":
        inference_fit).  factor="init": each group's init-kernel covariance at its start point; "fit": its least-squares
        covariance.  Returns {dc: PosteriorPool} as MCMC.sample_dr gives it for one group; chain j of group g draws from the Philox
        stream (seed, g * n_chains (rounded) + j).  The `inference` path is not touched."""
        n_chains, n_iter, ipl = int(n_chains), int(n_iter), int(iters_per_launch)
        nburn = n_iter // 2 if nburn is None else int(nburn)
        if n_chains < 1 or n_iter < 1 or not 0 <= nburn < n_iter or int(thin) < 1 or ipl < 1:
            raise ValueError("n_chains >= 1, n_iter >= 1, 0 <= nburn < n_iter, thin >= 1, iters_per_launch >= 1")
        if start not in ("fit", "qstart"):
            raise ValueError(f"start is 'fit' or 'qstart', not {start!r}")
        if factor not in ("init", "fit"):
            raise ValueError(f"factor is 'init' or 'fit', not {factor!r}")
        n, G = self.model.num_tsteps, len(self.dc_list)
        data = np.ascontiguousarray(np.asarray(self.data, dtype=np.float64).reshape(G, n))
        probes = [MCMC(self.model, data[g], self.dc_list[g], self.qpriors, self.qstart, nsamples=10) for g in range(G)]
        lo, hi = probes[0].qstart_limits[:, 0], probes[0].qstart_limits[:, 1]
        d = probes[0].n_params
        starts = np.tile(np.asarray(self.qstart, dtype=np.float64).reshape(1, d), (G, 1))
        est = self.inference_fit(seed=seed, mem=mem, device=device) if "fit" in (start, factor) else None
        if start == "fit":
            starts = np.stack([est[float(dc)]["q"] for dc in self.dc_list])
        out = {}
        with Engine(mem=mem, device=device) as eng:
            per = -(-n_chains // eng.block_threads) * eng.block_threads if G > 1 else n_chains
            eng.set_model(self.model, getattr(self.model, "substeps", 1))
            if factor == "init":
                L = np.stack([probes[g]._dr_init_factor(eng, starts[g]) for g in range(G)])
            else:
                L = np.stack([np.linalg.cholesky(est[float(dc)]["cov"]) for dc in self.dc_list])
            res = eng.dr(np.repeat(starts, per, axis=0), data, lo, hi, L, n_iter, gamma=gamma, stages=stages, seed=seed, iters_per_launch=ipl,
                         keep=n_iter - nburn, thin=thin, adapt_launches=nburn // ipl if adapt else 0)
            std2 = res.std2(engine=eng, kept=True)
            eng.sync()
        self.dr_result = res
        for g, dc in enumerate(self.dc_list):
            s = slice(g * per, (g + 1) * per)
            part = DrResult(res.q[s], res.l[s], [c[s] for c in (res.accepted1, res.accepted2, res.outbox1, res.outbox2, res.stuck)], res.n_iter,
                            res.trace_q[:, s], res.trace_l[:, s], res.iterations, res.chol[g:g + 1], res.gamma, res.stages, res.shape, res.seed,
                            res.offset + g * per, res.iter0)
            out[float(dc)] = MCMC._dr_pool(part, std2[:, s], nburn)
        return out

    def inference_law(self, n_chains=256, n_iter=200, nburn=None, n_starts=64, gamma=0.2, stages=2, adapt=True, seed=0, mem="device", device=-1, thin=1,
                      iters_per_launch=16, **fit_kw):
        """Additive: the laboratory workflow for every series of dc_list under the model's state law, observable and loading
        history — the least-squares fit of all groups in ONE call (Engine.law_fit; each group n_starts start points, MCMC.fit_law's),
        then MCMC.sample_law per group from its best point (start: that point for every chain; factor="gn" there).  Returns
        ({dc: dict(q, ssq, cov, stderr, status, iters, index)} in inference_fit's shape, {dc: PosteriorPool}); the FitResult of all
        starts is kept in self.fit_result.  The fit runs in host memory as inference_fit does by default, the sampler in `mem`.  fit_kw: Engine.law_fit's fd_rel_step, ftol, max_iter.  The `inference` path is not touched."""
        n_chains, n_iter = int(n_chains), int(n_iter)
        if n_chains < 1 or n_iter < 1:
            raise ValueError("n_chains >= 1, n_iter >= 1")
        n, G = self.model.num_tsteps, len(self.dc_list)
        data = np.ascontiguousarray(np.asarray(self.data, dtype=np.float64).reshape(G, n))
        probes = [MCMC(self.model, data[g], self.dc_list[g], self.qpriors, self.qstart, nsamples=10, verbose=False) for g in range(G)]
        with Engine(mem="host", device=device) as eng:
            eng.set_model(self.model, getattr(self.model, "substeps", 1))
            q0, lo, hi = probes[0]._fit_starts(eng, n_starts, seed)
            res = eng.law_fit(probes[0]._law(), probes[0]._observable(), np.tile(q0, (G, 1)), data, lo, hi, **fit_kw)
            eng.sync()
        self.fit_result, fits, pools = res, {}, {}
        for g, dc in enumerate(self.dc_list):
            i = res.best(g)
            cov = res.covariance(i)
            fits[float(dc)] = {"q": res.q[i].copy(), "ssq": float(res.ssq[i]), "cov": cov, "stderr": np.sqrt(np.diag(cov)),
                               "status": int(res.status[i]), "iters": int(res.iters[i]), "index": i}
        for g, dc in enumerate(self.dc_list):
            pools[float(dc)] = probes[g].sample_law(n_chains, n_iter, nburn=nburn, start=np.tile(fits[float(dc)]["q"], (n_chains, 1)), factor="gn",
                                                    gamma=gamma, stages=stages, adapt=adapt, seed=seed, mem=mem, device=device, thin=thin,
                                                    iters_per_launch=iters_per_launch)
        self.posteriors = {dc: pool.pooled() for dc, pool in pools.items()}
        return fits, pools

    @measure_execution_time
    def inference(self, nsamples):
        data = self.prepare_data(self.data)
        for dc in self.dc_list:
            self.perform_sampling_and_plotting(data, dc, nsamples, None)
        return
