#!/usr/bin/env python3
"""
Cost of the multi-start Levenberg-Marquardt fit (include/rsf_fit.h) on the GPU: one process, device-memory engine, median of 5 after
a warm-up.
    python tools/fit_bench.py [--out profiles/fit/fit_bench.json] [--quick]
  iteration  one rsf_fit_run iteration per start against rsf_mcmc_init (the bare group solve: the same lanes, the same solve, no
             iteration around it) at the same n, d and nsteps — 65 536 starts, nsteps 2000 — the init timed before and after in
             the same process.  Every timed launch starts from the same state, in which every start is RUNNING.  Two figures:
             "same_points" — lam = 1e9, so that the trial point is the start point to nine digits and the solve is the one
             rsf_mcmc_init runs: the kernel's own overhead; "first_four" — the first four iterations from lam = 1e-3 in one
             launch, whose trial points run to the box's edges where the solves are stiff: what a fit pays at its beginning.
  whole      Engine.fit (RSF.inference_fit, 64 starts per group) on main.py's problem, five true Dc from 100 to 5000 at nsteps 500,
             next to the burn-in sample_batched's chains need from qstart = 1000 on the same data: per group the first iteration
             at which the median chain of 256 lies within three standard errors of the least-squares estimate.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import bayesian_markov_chain_monte_carlo_amd as pkg  # noqa: E402

BOX = {1: ([0.0], [1.0e4]), 3: ([0.0, 1e-3, 1e-3], [1.0e4, 0.1, 0.1])}


def median_time(fn, sync, reps=5, before=None):
    ts = []
    for r in range(reps + 1):  # the first is the warm-up
        arg = before() if before else None
        sync()
        t = time.perf_counter()
        fn(arg) if before else fn()
        sync()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts[1:]))


def bench_iteration(eng, n, nsteps, d, n_iter=4):
    import torch

    model = pkg.RateStateModel(number_time_steps=nsteps)
    eng.set_model(model, 1)
    truth = np.asarray(eng.forward([1000.0])[1].cpu())[:, 0]
    data = torch.as_tensor(truth + 0.01 * np.abs(truth).max() * np.random.default_rng(1).standard_normal(truth.size), device=f"cuda:{eng.device}")
    lo, hi = BOX[d]
    rng = np.random.default_rng(2)
    q0 = rng.uniform(300.0, 3000.0, (n, 1))
    if d == 3:
        q0 = np.concatenate([q0, rng.uniform(0.009, 0.013, (n, 1)), rng.uniform(0.0145, 0.0158, (n, 1))], axis=1)
    q0 = eng._in(q0)
    fd = 1e-6 if d == 1 else 1e-4
    init = lambda: eng.mcmc_init(q0, data, lo, hi, n0=0.0, fd_rel_step=fd, adapt_mode="none")
    t0 = median_time(init, eng.sync)
    tn = median_time(lambda: eng.fit_normal(q0, data, fd), eng.sync)
    ssq, g, H = eng.fit_normal(q0, data, fd)
    out = {"n": n, "nsteps": nsteps, "d": d, "fit_normal_s": tn}
    for name, lam0, k in (("same_points", 1e9, 1), ("first_four", pkg._abi.FIT_LAM0, n_iter)):
        base = (q0, ssq, g, H, eng._in(np.full(n, lam0)), eng._ints(np.zeros(n)), eng._ints(np.zeros(n)))
        fresh = lambda: [x.clone() for x in base]
        run = lambda s: eng.fit_run(s[0], data, lo, hi, s[1], s[2], s[3], s[4], s[5], s[6], k, fd, 0.0)  # ftol 0: nothing converges
        tr = median_time(run, eng.sync, before=fresh) / k
        s = fresh()
        run(s)
        eng.sync()
        out[name] = {"n_iter": k, "fit_run_per_iteration_s": tr, "running_after": float((s[5] == pkg._abi.FIT_RUNNING).double().mean().item()),
                     "accepted": float((s[4] < lam0).double().mean().item())}
    t1 = median_time(init, eng.sync)
    out["mcmc_init_s"] = [t0, t1]
    for name in ("same_points", "first_four"):
        out[name]["ratio_to_mcmc_init"] = out[name]["fit_run_per_iteration_s"] / (0.5 * (t0 + t1))
    return out


def bench_whole(n_starts=64, chains=256, n_iters=2000):
    if os.path.join(ROOT, "bayesian-markov-chain-monte-carlo_amd") not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, "bayesian-markov-chain-monte-carlo_amd"))
    np.random.seed(0)
    problem = pkg.RSF(number_slip_values=5, lowest_slip_value=100.0, largest_slip_value=5000.0, qstart=1000.0, qpriors=["Uniform", 0.0, 10000.0])
    problem.model = pkg.RateStateModel(number_time_steps=500)
    problem.data = problem.generate_time_series()
    problem.inference_fit(n_starts=n_starts, mem="device")  # warm-up: library load, first launches
    t = time.perf_counter()
    fits = problem.inference_fit(n_starts=n_starts, mem="device")
    t_fit = time.perf_counter() - t
    res = problem.fit_result
    G, n = len(problem.dc_list), problem.model.num_tsteps
    data = np.ascontiguousarray(np.asarray(problem.data).reshape(G, n))
    out = {"n_starts": n_starts, "engine_fit_s": t_fit, "group_solves": int(res.iters.sum() + res.iters.size),
           "status_counts": np.bincount(res.status, minlength=4).tolist(), "iters_max": int(res.iters.max()),
           "groups": {str(dc): {"q": float(f["q"][0]), "stderr": float(f["stderr"][0]), "ssq": f["ssq"], "status": f["status"], "iters": f["iters"]}
                      for dc, f in fits.items()}}
    with pkg.Engine(mem="device") as eng:
        eng.set_model(problem.model, 1)
        eng.mcmc_init(np.full((G * chains, 1), 1000.0), data, [0.0], [1.0e4], seed=0, n0=0.01, prior_len=3, adapt_mode="none")
        eng.sync()
        t = time.perf_counter()
        tq, _, ta = eng.mcmc_run(n_iters)
        eng.sync()
        t_run = time.perf_counter() - t
        tq, ta = np.asarray(tq.cpu())[:, :, 0], np.asarray(ta.cpu())
    burn = {}
    for g, dc in enumerate(problem.dc_list):
        f = fits[float(dc)]
        z = np.median(np.abs(tq[:, g * chains:(g + 1) * chains] - f["q"][0]) / f["stderr"][0], axis=1)
        hit = np.flatnonzero(z <= 3.0)
        burn[str(float(dc))] = {"burn_in_iterations": int(hit[0]) + 1 if hit.size else None, "accept_rate": float(ta[:, g * chains:(g + 1) * chains].mean()),
                                "median_z_at_end": float(z[-1])}
    out["sample_batched"] = {"chains_per_group": chains, "n_iters": n_iters, "mcmc_run_s": t_run, "groups": burn}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="4096 starts, nsteps 500")
    args = ap.parse_args()
    n, nsteps = (4096, 500) if args.quick else (65536, 2000)
    out = {"device": None, "build_id": pkg._abi.load().rsf_build_id().decode(), "iteration": [], "whole": None}
    with pkg.Engine(mem="device") as eng:
        import torch

        out["device"] = torch.cuda.get_device_name(eng.device)
        for d in (1, 3):
            out["iteration"].append(bench_iteration(eng, n, nsteps, d))
            print(json.dumps(out["iteration"][-1]), flush=True)
    out["whole"] = bench_whole(n_iters=500 if args.quick else 2000)
    print(json.dumps(out["whole"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
