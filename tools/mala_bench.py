#!/usr/bin/env python3
"""
Cost and efficiency of the Gauss-Newton manifold MALA sampler (include/rsf_mala.h) on the GPU: one process, device-memory engine,
median of 5 after a warm-up.
    python tools/mala_bench.py [--out profiles/mala/mala_bench.json] [--quick]
  cost        one rsf_mala_run iteration per chain against rsf_fit_normal of the same points (the bare group solve: the same
              lanes, the same solve, nothing around it) at the same n, d and nsteps — 65 536 chains, nsteps 2000 — rsf_fit_normal
              timed before and after in the same process.  Every timed launch of four iterations starts from the same state.  Two
              figures: "eps_1" — the default step, whose proposals are the sampler's own (the share inside the box is recorded:
              a wave without one skips its solve); "same_points" — eps = 1e-6, so that every proposal is its chain's point to
              six digits and the solve is the one rsf_fit_normal runs: the iteration's own overhead.
  efficiency  bulk ESS (Engine.rank_diagnostics) of the kept draws per forward solve of the kept phase — a MALA iteration counts
              1 + d solves per chain whether its proposal left the box or not, a random-walk iteration one — on main.py's problem
              (five true Dc from 100 to 5000, nsteps 500), 256 chains per group: RSF.inference_mala (start="fit") against
              MCMC.sample_batched with its defaults from qstart = 1000, d = 1; and at d = 3 (Dc, a, b) on the Dc_true = 1000 series
              for Dc, a and Dc a, MALA at several eps.
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

BOX = {1: ([0.0], [1.0e4]), 3: ([0.0, 0.005, 0.005], [1.0e4, 0.02, 0.03])}


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


def bench_cost(eng, n, nsteps, d, n_iter=4):
    import torch

    model = pkg.RateStateModel(number_time_steps=nsteps)
    eng.set_model(model, 1)
    truth = np.asarray(eng.forward([1000.0])[1].cpu())[:, 0]
    data = torch.as_tensor(truth + 0.01 * np.abs(truth).max() * np.random.default_rng(1).standard_normal(truth.size), device=f"cuda:{eng.device}")
    lo, hi = BOX[d]
    fd = 1e-6 if d == 1 else 1e-4
    # the chains' points: the least-squares estimate, then twenty iterations of the sampler itself
    start = eng.fit([[1000.0] if d == 1 else [1000.0, model.a, model.b]], data, lo, hi, fd_rel_step=fd)
    res = eng.mala(np.tile(start.q[start.best()], (n, 1)), data, lo, hi, 20, seed=1, fd_rel_step=fd)
    q0 = eng._in(res.q)
    normal = lambda: eng.fit_normal(q0, data, fd)
    t0 = median_time(normal, eng.sync)
    ssq, g, H = eng.fit_normal(q0, data, fd)
    out = {"n": n, "nsteps": nsteps, "d": d, "warm_up": {"accept_rate": res.accept_rate, "outbox": float(res.outbox.mean() / 20)}}
    for name, eps in (("eps_1", 1.0), ("same_points", 1e-6)):
        base = (q0, ssq, g, H, *(eng._ints(np.zeros(n)) for _ in range(3)))
        fresh = lambda: [x.clone() for x in base]
        run = lambda s: eng.mala_run(s[0], s[1], s[2], s[3], data, lo, hi, n_iter, s[4], s[5], s[6], eps=eps, seed=2, fd_rel_step=fd)
        tr = median_time(run, eng.sync, before=fresh) / n_iter
        s = fresh()
        run(s)
        eng.sync()
        out[name] = {"n_iter": n_iter, "mala_run_per_iteration_s": tr, "accepted": float(s[4].double().mean().item()) / n_iter,
                     "outbox": float(s[5].double().mean().item()) / n_iter, "stuck": int(s[6].sum().item())}
    t1 = median_time(normal, eng.sync)
    out["fit_normal_s"] = [t0, t1]
    for name in ("eps_1", "same_points"):
        out[name]["ratio_to_fit_normal"] = out[name]["mala_run_per_iteration_s"] / (0.5 * (t0 + t1))
    return out


def _ess(eng, samples, columns):
    """bulk ESS, rank-normalised R-hat and the mean of the listed series of kept draws (n_keep, C)"""
    out = {}
    for name, x in columns.items():
        r = eng.rank_diagnostics(np.ascontiguousarray(x[:, :, None]))[0]
        out[name] = {"ess_bulk": float(r["ess_bulk"]), "rhat": float(r["rhat"]), "mean": float(x.mean()), "sd": float(x.std())}
    return out


def bench_d1(chains=256, mala_iter=200, rw_iter=2000):
    if os.path.join(ROOT, "bayesian-markov-chain-monte-carlo_amd") not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, "bayesian-markov-chain-monte-carlo_amd"))
    np.random.seed(0)
    problem = pkg.RSF(number_slip_values=5, lowest_slip_value=100.0, largest_slip_value=5000.0, qstart=1000.0, qpriors=["Uniform", 0.0, 10000.0])
    problem.model = pkg.RateStateModel(number_time_steps=500)
    problem.data = problem.generate_time_series()
    G, n = len(problem.dc_list), problem.model.num_tsteps
    data = np.ascontiguousarray(np.asarray(problem.data).reshape(G, n))
    t = time.perf_counter()
    pools = problem.inference_mala(n_chains=chains, n_iter=mala_iter, start="fit", seed=0)
    t_mala = time.perf_counter() - t
    out = {"chains_per_group": chains, "mala": {"n_iter": mala_iter, "wall_s_with_fit": t_mala, "fit_group_solves": int(problem.fit_result.iters.sum() + problem.fit_result.iters.size)},
           "sample_batched": {"n_iters": rw_iter}, "groups": {}}
    with pkg.Engine(mem="device") as eng:
        for g, dc in enumerate(problem.dc_list):
            pool = pools[float(dc)]
            solves = pool.samples.shape[0] * chains * 2
            m = _ess(eng, pool.samples, {"Dc": pool.samples[:, :, 0]})["Dc"]
            m.update({"accept_rate": pool.accept_rate, "out_of_bounds": pool.stats["out_of_bounds"] / (mala_iter * chains), "stuck": pool.stats["stuck"],
                      "kept_solves": solves, "ess_per_solve": m["ess_bulk"] / solves})
            mc = pkg.MCMC(problem.model, data[g], float(dc), ["Uniform", 0.0, 10000.0], 1000.0, nsamples=rw_iter, verbose=False)
            rw = mc.sample_batched(chains, seed=0)
            solves = rw.samples.shape[0] * chains
            r = _ess(eng, rw.samples, {"Dc": rw.samples[:, :, 0]})["Dc"]
            r.update({"accept_rate": float(rw.accept_rate), "out_of_bounds": 1.0 - rw.stats["evaluated"] / (rw_iter * chains), "kept_solves": solves,
                      "ess_per_solve": r["ess_bulk"] / solves})
            out["groups"][str(float(dc))] = {"mala": m, "sample_batched": r, "mala_over_sample_batched": m["ess_per_solve"] / r["ess_per_solve"]}
            print(json.dumps({str(float(dc)): out["groups"][str(float(dc))]}), flush=True)
    return out


def bench_d3(chains=256, mala_iter=400, rw_iter=4000, eps_list=(1.0, 0.3, 0.1, 0.03, 0.01)):
    model = pkg.RateStateModel(number_time_steps=500)
    lo, hi = BOX[3]
    cols = lambda s: {"Dc": s[:, :, 0], "a": s[:, :, 1], "Dc*a": s[:, :, 0] * s[:, :, 1]}
    out = {"chains": chains, "mala": {}, "sample_batched": None}
    with pkg.Engine(mem="device") as eng:
        eng.set_model(model, 1)
        truth = np.asarray(eng.forward([1000.0])[1].cpu())[:, 0]
        data = truth + 0.01 * np.abs(truth).max() * np.random.default_rng(1).standard_normal(truth.size)
        mc = pkg.MCMC(model, data, 1000.0, [["Uniform", l, h] for l, h in zip(lo, hi)], [1000.0, model.a, model.b], nsamples=rw_iter, verbose=False)
        for eps in eps_list:
            pool = mc.sample_mala(chains, mala_iter, start="fit", seed=0, eps=eps)
            solves = pool.samples.shape[0] * chains * 4
            m = _ess(eng, pool.samples, cols(pool.samples))
            for v in m.values():
                v["ess_per_solve"] = v["ess_bulk"] / solves
            out["mala"][str(eps)] = {"n_iter": mala_iter, "accept_rate": pool.accept_rate, "out_of_bounds": pool.stats["out_of_bounds"] / (mala_iter * chains),
                                     "stuck": pool.stats["stuck"], "kept_solves": solves, "series": m}
            print(json.dumps({"d3 mala eps": eps, **out["mala"][str(eps)]}), flush=True)
        rw = mc.sample_batched(chains, seed=0)
        solves = rw.samples.shape[0] * chains
        r = _ess(eng, rw.samples, cols(rw.samples))
        for v in r.values():
            v["ess_per_solve"] = v["ess_bulk"] / solves
        out["sample_batched"] = {"n_iters": rw_iter, "accept_rate": float(rw.accept_rate), "out_of_bounds": 1.0 - rw.stats["evaluated"] / (rw_iter * chains),
                                 "kept_solves": solves, "series": r}
        print(json.dumps({"d3 sample_batched": out["sample_batched"]}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="4096 chains, nsteps 500, shorter runs")
    args = ap.parse_args()
    n, nsteps = (4096, 500) if args.quick else (65536, 2000)
    out = {"device": None, "build_id": pkg._abi.load().rsf_build_id().decode(), "cost": [], "d1": None, "d3": None}
    with pkg.Engine(mem="device") as eng:
        import torch

        out["device"] = torch.cuda.get_device_name(eng.device)
        for d in (1, 3):
            out["cost"].append(bench_cost(eng, n, nsteps, d))
            print(json.dumps(out["cost"][-1]), flush=True)
    out["d1"] = bench_d1(**(dict(mala_iter=60, rw_iter=400) if args.quick else {}))
    out["d3"] = bench_d3(**(dict(mala_iter=60, rw_iter=400) if args.quick else {}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
