#!/usr/bin/env python3
"""
Cost and efficiency of the two-stage delayed-rejection sampler (include/rsf_dr.h) on the GPU: one process, device-memory engine,
median of 5 after a warm-up.
    python tools/dr_bench.py [--out profiles/dr/dr_bench.json] [--quick]
  cost        rsf_dr_run with stages = 1 against rsf_smc_move(beta = 1) with steps = n_iter on the same points, the same factor and
              the same draws (the two are bit-identical: the same solves), 65 536 chains, nsteps 2000, d = 1 and 3; rsf_smc_move
              timed before and after.  Then stages = 2 from the same state: ms per iteration, the solves it executed
              (DrResult.n_solves' identity on the counters) and ms per executed solve per chain-slot against the baseline's — what
              the half-empty second solve costs.  The points are a sample of the target (twenty iterations of the sampler itself
              from a ball around the least-squares estimate), the factor is the adapted one of that sample.
  efficiency  bulk ESS (Engine.rank_diagnostics) of the kept half per forward solve EXECUTED in that half, on main.py's five groups
              (true Dc 100 .. 5000, nsteps 500, box (0, 1e4), every chain started at qstart = 1000), 256 chains each:
              delayed rejection with factor = "init" (the init kernel's covariance at qstart, what sample_batched proposes from),
              adaptation off and on, 1000 iterations; MCMC.sample_batched with its defaults, 2000 iterations, per iteration (the
              figure of DESIGN 4j's table: a proposal outside the box counts as a solve slot) and per executed solve.
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


def bench_cost(eng, n, nsteps, d, n_iter=4, gamma=0.2):
    import torch

    model = pkg.RateStateModel(number_time_steps=nsteps)
    eng.set_model(model, 1)
    truth = np.asarray(eng.forward([1000.0])[1].cpu())[:, 0]
    data = torch.as_tensor(truth + 0.01 * np.abs(truth).max() * np.random.default_rng(1).standard_normal(truth.size), device=f"cuda:{eng.device}")
    lo, hi = (np.asarray(x) for x in BOX[d])
    start = eng.fit([[1000.0] if d == 1 else [1000.0, model.a, model.b]], data, lo, hi)
    centre = start.q[start.best()]
    L0 = np.diag(np.maximum(1e-3 * np.abs(centre), 1e-6 * (hi - lo)))
    q0 = np.clip(centre + 1e-3 * np.abs(centre) * np.random.default_rng(2).standard_normal((n, d)), lo + 1e-9 * (hi - lo), hi - 1e-9 * (hi - lo))
    res = eng.dr(q0, data, lo, hi, L0, 20, gamma=gamma, seed=1, keep=0, iters_per_launch=4, adapt_launches=5)
    q, l, chol = eng._in(res.q), eng._in(res.l), res.chol[0]
    move = lambda: eng.smc_move(q, l, data, lo, hi, chol, 1.0, seed=3, steps=n_iter)
    t0 = median_time(move, eng.sync) / n_iter
    fresh = lambda: [q.clone(), l.clone(), [eng._ints(np.zeros(n)) for _ in range(5)]]
    out = {"n": n, "nsteps": nsteps, "d": d, "n_iter": n_iter, "gamma": gamma, "warm_up_accept_rates": list(res.accept_rates)}
    for stages in (1, 2):
        run = lambda s: eng.dr_run(s[0], s[1], data, lo, hi, chol, n_iter, s[2], gamma=gamma, stages=stages, seed=3)
        t = median_time(run, eng.sync, before=fresh) / n_iter
        s = fresh()
        run(s)
        eng.sync()
        a1, a2, o1, o2, st = (int(c.sum().item()) for c in s[2])
        solves = (n * n_iter - st - o1) + ((n * n_iter - st - a1 - o2) if stages == 2 else 0)
        out[f"stages{stages}"] = {"per_iteration_s": t, "accepted1": a1 / (n * n_iter), "accepted2": a2 / (n * n_iter), "outbox1": o1 / (n * n_iter),
                                  "outbox2": o2 / (n * n_iter), "stuck": st, "solves_per_chain_iteration": solves / (n * n_iter)}
    t1 = median_time(move, eng.sync) / n_iter
    base = 0.5 * (t0 + t1)
    out["smc_move_per_step_s"] = [t0, t1]
    out["stages1_over_smc_move"] = out["stages1"]["per_iteration_s"] / base
    out["stages2_over_smc_move"] = out["stages2"]["per_iteration_s"] / base
    # per executed solve: the time of an iteration over the solves a chain made in it, against the baseline's one slot per step
    out["stages2_per_solve_over_smc_move"] = out["stages2"]["per_iteration_s"] / out["stages2"]["solves_per_chain_iteration"] / base
    return out


def _ess(eng, x):
    r = eng.rank_diagnostics(np.ascontiguousarray(x[:, :, None]))[0]
    return {"ess_bulk": float(r["ess_bulk"]), "rhat": float(r["rhat"]), "mean": float(x.mean()), "sd": float(x.std())}


def bench_d1(chains=256, dr_iter=1000, rw_iter=2000, gamma=0.2):
    if os.path.join(ROOT, "bayesian-markov-chain-monte-carlo_amd") not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, "bayesian-markov-chain-monte-carlo_amd"))
    np.random.seed(0)
    problem = pkg.RSF(number_slip_values=5, lowest_slip_value=100.0, largest_slip_value=5000.0, qstart=1000.0, qpriors=["Uniform", 0.0, 10000.0])
    problem.model = pkg.RateStateModel(number_time_steps=500)
    problem.data = problem.generate_time_series()
    data = np.asarray(problem.data).reshape(len(problem.dc_list), -1)
    lo, hi = BOX[1]
    out = {"chains_per_group": chains, "dr_iter": dr_iter, "rw_iter": rw_iter, "gamma": gamma, "groups": {}}
    with pkg.Engine(mem="device") as eng:
        eng.set_model(problem.model, 1)
        for g, dc in enumerate(problem.dc_list):
            mc = pkg.MCMC(problem.model, data[g], float(dc), ["Uniform", 0.0, 10000.0], 1000.0, nsamples=rw_iter, verbose=False)
            L = mc._dr_init_factor(eng, [1000.0])
            eng.set_model(problem.model, 1)
            row = {"init_factor": float(L[0, 0])}
            for name, adapt in (("dr", 0), ("dr_adapted", (dr_iter // 2) // 16)):
                # the burn-in, then the kept half as a continuation: its counters are the kept half's alone
                burn = eng.dr(np.full((chains, 1), 1000.0), data[g], lo, hi, L, dr_iter // 2, gamma=gamma, seed=0, keep=0, adapt_launches=adapt)
                kept = eng.dr(burn.q, data[g], lo, hi, burn.chol, dr_iter - dr_iter // 2, gamma=gamma, seed=0, iter0=dr_iter // 2 + 1, l0=burn.l)
                m = _ess(eng, kept.trace_q[:, :, 0])
                slots = kept.n_iter * chains
                m.update({"factor": float(burn.chol[0, 0, 0]), "accept_rate1": kept.accept_rates[0], "accept_rate2": kept.accept_rates[1],
                          "outbox1": kept.outbox_rates[0], "outbox2": kept.outbox_rates[1], "stuck": int(kept.stuck.sum()), "kept_iterations": slots,
                          "kept_solves": kept.n_solves, "ess_per_solve": m["ess_bulk"] / kept.n_solves, "ess_per_iteration": m["ess_bulk"] / slots})
                row[name] = m
            rw = mc.sample_batched(chains, seed=0)
            slots = rw.samples.shape[0] * chains
            r = _ess(eng, rw.samples[:, :, 0])
            oob = 1.0 - rw.stats["evaluated"] / (rw_iter * chains)
            r.update({"accept_rate": float(rw.accept_rate), "out_of_bounds": oob, "kept_iterations": slots, "ess_per_iteration": r["ess_bulk"] / slots,
                      "ess_per_solve": r["ess_bulk"] / (slots * (1.0 - oob))})
            row["sample_batched"] = r
            row["dr_over_sample_batched_per_solve"] = row["dr"]["ess_per_solve"] / r["ess_per_solve"]
            row["dr_over_sample_batched_per_iteration_slot"] = row["dr"]["ess_per_solve"] / r["ess_per_iteration"]
            out["groups"][str(float(dc))] = row
            print(json.dumps({str(float(dc)): row}), flush=True)
            eng.set_model(problem.model, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="4096 chains, nsteps 500, shorter runs")
    ap.add_argument("--cost-only", action="store_true", help="the cost figures alone")
    args = ap.parse_args()
    n, nsteps = (4096, 500) if args.quick else (65536, 2000)
    out = {"device": None, "build_id": pkg._abi.load().rsf_build_id().decode(), "cost": [], "d1": None}
    with pkg.Engine(mem="device") as eng:
        import torch

        out["device"] = torch.cuda.get_device_name(eng.device)
        for d in (1, 3):
            out["cost"].append(bench_cost(eng, n, nsteps, d))
            print(json.dumps(out["cost"][-1]), flush=True)
    if not args.cost_only:
        out["d1"] = bench_d1(**(dict(dr_iter=128, rw_iter=200) if args.quick else {}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
