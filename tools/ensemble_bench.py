#!/usr/bin/env python3
"""
Cost and efficiency of the affine-invariant ensemble sampler in islands (include/rsf_ensemble.h) on the GPU: one process,
device-memory engine, median of 5 after a warm-up.
    python tools/ensemble_bench.py [--out profiles/ensemble/ensemble_bench.json] [--quick]
  cost        one rsf_ensemble_run iteration per walker (two half-steps: every lane solves twice) against rsf_smc_move with
              steps = n_iter on the same n points in the same process — the same solves in the same arrangement, one lane per
              point — 65 536 and 524 288 walkers, nsteps 2000, d = 1 and 3; rsf_smc_move timed before and after.  An ensemble
              iteration moves each walker once and so costs n solves, like one rsf_smc_move step: the figure is per iteration against
              per step.  The ensemble launch has n / 2 lanes that solve twice in sequence, rsf_smc_move's n lanes that solve once: the
              smaller size, which does not fill the machine with either, measures that; the larger one measures throughput.
  efficiency  bulk ESS (Engine.rank_diagnostics) of the kept draws per forward solve of the kept phase (one per walker and
              iteration, whether the proposal left the box or not), rank R-hat over walkers, nested R-hat over islands
              (PosteriorPool.diagnostics), acceptance, the share outside the box and the pool's mean — on DESIGN 4j's problems:
              d = 1, main.py's five groups at nsteps 500, one island of 512 walkers per group (RSF.inference_ensemble, start="fit");
              d = 3 (Dc, a, b) on the Dc_true = 1000 series with 1 % noise, four islands, with and without log coordinates, from
              the fit's point and from SMC's particles.
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
    lo, hi = (np.asarray(x) for x in BOX[d])
    mask = 0b011 if d == 3 else 0
    # the walkers: a ball around the least-squares estimate, then twenty iterations of the sampler itself
    start = eng.fit([[1000.0] if d == 1 else [1000.0, model.a, model.b]], data, lo, hi)
    q0 = pkg.MCMC._ensemble_ball(start.q[start.best()], lo, hi, mask, n, np.random.default_rng(2))
    res = eng.ensemble(q0, data, lo, hi, 20, log_coords=mask, seed=1, keep=0)
    q, l = eng._in(res.q), eng._in(res.l)
    chol = np.linalg.cholesky((2.38 ** 2 / d) * np.atleast_2d(np.cov(res.q.T)) + np.diag((1e-6 * (hi - lo)) ** 2))
    move = lambda: eng.smc_move(q, l, data, lo, hi, chol, 1.0, seed=3, steps=n_iter)
    t0 = median_time(move, eng.sync) / n_iter
    base = (q, l, *(eng._ints(np.zeros(n)) for _ in range(3)))
    fresh = lambda: [x.clone() for x in base]
    run = lambda s: eng.ensemble_run(s[0], s[1], data, lo, hi, n_iter, s[2], s[3], s[4], log_coords=mask, seed=2)
    tr = median_time(run, eng.sync, before=fresh) / n_iter
    s = fresh()
    run(s)
    eng.sync()
    acc = eng.smc_move(q, l, data, lo, hi, chol, 1.0, seed=3, steps=n_iter)[2]
    t1 = median_time(move, eng.sync) / n_iter
    return {"n": n, "nsteps": nsteps, "d": d, "logmask": mask, "n_iter": n_iter, "island_size": eng.island_size,
            "warm_up": {"accept_rate": res.accept_rate, "outbox": res.outbox_rate},
            "ensemble_run_per_iteration_s": tr, "accepted": float(s[2].double().mean().item()) / n_iter,
            "outbox": float(s[3].double().mean().item()) / n_iter, "stuck": int(s[4].sum().item()),
            "smc_move_per_step_s": [t0, t1], "smc_move_accept_rate": float(np.mean(acc)) / n, "ratio_to_smc_move": tr / (0.5 * (t0 + t1))}


def _series(eng, pool, columns):
    """bulk ESS, rank R-hat over walkers, nested R-hat over islands, mean and SD of the listed series of kept draws (n_keep, n)"""
    out = {}
    solves = pool.samples.shape[0] * pool.samples.shape[1]
    for name, x in columns.items():
        x3 = np.ascontiguousarray(x[:, :, None])
        r = eng.rank_diagnostics(x3)[0]
        dg = eng.diagnostics(x3, superchain_size=pool.stats["island_size"])[0] if pool.stats["n_islands"] > 1 else {}
        out[name] = {"ess_bulk": float(r["ess_bulk"]), "ess_per_solve": float(r["ess_bulk"]) / solves, "rhat": float(r["rhat"]),
                     "nested_rhat": float(dg["nested_rhat"]) if "nested_rhat" in dg else None, "mean": float(x.mean()), "sd": float(x.std())}
    return out, solves


def _pool_row(eng, pool, columns, n_iter):
    series, solves = _series(eng, pool, columns)
    n = pool.stats["n_walkers"]
    return {"n_walkers": n, "n_islands": pool.stats["n_islands"], "n_iter": n_iter, "kept_rows": int(pool.samples.shape[0]), "kept_solves": solves,
            "accept_rate": pool.accept_rate, "out_of_bounds": pool.stats["out_of_bounds"] / (n_iter * n), "stuck": pool.stats["stuck"], "series": series}


def bench_d1(walkers=512, n_iter=200):
    if os.path.join(ROOT, "bayesian-markov-chain-monte-carlo_amd") not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, "bayesian-markov-chain-monte-carlo_amd"))
    np.random.seed(0)
    problem = pkg.RSF(number_slip_values=5, lowest_slip_value=100.0, largest_slip_value=5000.0, qstart=1000.0, qpriors=["Uniform", 0.0, 10000.0])
    problem.model = pkg.RateStateModel(number_time_steps=500)
    problem.data = problem.generate_time_series()
    t = time.perf_counter()
    pools = problem.inference_ensemble(n_walkers=walkers, n_iter=n_iter, start="fit", seed=0)
    out = {"wall_s_with_fit": time.perf_counter() - t, "groups": {}}
    with pkg.Engine(mem="device") as eng:
        for dc in problem.dc_list:
            pool = pools[float(dc)]
            out["groups"][str(float(dc))] = _pool_row(eng, pool, {"Dc": pool.samples[:, :, 0]}, n_iter)
            print(json.dumps({str(float(dc)): out["groups"][str(float(dc))]}), flush=True)
    return out


def bench_d3(walkers=2048, n_iter=400):
    model = pkg.RateStateModel(number_time_steps=500)
    lo, hi = BOX[3]
    cols = lambda s: {"Dc": s[:, :, 0], "a": s[:, :, 1], "b": s[:, :, 2], "Dc*a": s[:, :, 0] * s[:, :, 1]}
    out = {}
    with pkg.Engine(mem="device") as eng:
        eng.set_model(model, 1)
        truth = np.asarray(eng.forward([1000.0])[1].cpu())[:, 0]
        data = truth + 0.01 * np.abs(truth).max() * np.random.default_rng(1).standard_normal(truth.size)
        mc = pkg.MCMC(model, data, 1000.0, [["Uniform", l, h] for l, h in zip(lo, hi)], [1000.0, model.a, model.b], nsamples=10, verbose=False)
        for start in ("fit", "smc"):
            for name, coords in (("log", (True, True, False)), ("plain", (False, False, False))):
                pool = mc.sample_ensemble(walkers, n_iter, start=start, log_coords=coords, seed=0)
                row = _pool_row(eng, pool, cols(pool.samples), n_iter)
                out[f"{start} {name}"] = row
                print(json.dumps({f"d3 {start} {name}": row}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="4096 walkers, nsteps 500, shorter runs")
    ap.add_argument("--cost-only", action="store_true", help="the cost figures alone")
    args = ap.parse_args()
    sizes, nsteps = ((4096,), 500) if args.quick else ((65536, 524288), 2000)
    out = {"device": None, "build_id": pkg._abi.load().rsf_build_id().decode(), "cost": [], "d1": None, "d3": None}
    with pkg.Engine(mem="device") as eng:
        import torch

        out["device"] = torch.cuda.get_device_name(eng.device)
        for n in sizes:
            for d in (1, 3):
                out["cost"].append(bench_cost(eng, n, nsteps, d))
                print(json.dumps(out["cost"][-1]), flush=True)
    if not args.cost_only:
        out["d1"] = bench_d1(**(dict(n_iter=40) if args.quick else {}))
        out["d3"] = bench_d3(**(dict(n_iter=60) if args.quick else {}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
