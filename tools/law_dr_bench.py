#!/usr/bin/env python3
"""
Cost of the fused delayed-rejection sampler under a state law (include/rsf_law_dr.h) on the GPU, against its own bare solve and
against the split path it replaces: recorded, not gated.
    python tools/law_dr_bench.py [--out profiles/law_dr/law_dr_bench.json] [--quick]
tools/observe_bench.py's method: one process, device-memory engine, every call warmed up, then the calls timed in turn, `rounds`
times over, each timing a host clock around one call that ends in a device synchronise; reported: the median over the rounds
with its spread (min, max).  Shape: `chains` chains (65 536, and 256 where launches and copies dominate) at nsteps 2000 under the
step history, friction data of the truth (Dc, a, b) = (20, 0.011, 0.014) with noise 5 % of the excursion, d = 1 and d = 3, both
laws; the chains are a sample of the target (16 iterations of the sampler itself from a ball around the truth), the factor
law_gn_factor's at the truth.  Timed, K = 4 iterations per call:
  solve     rsf_law_observe in SSq mode on the chains' points: the bare solve, one per chain
  stages1   rsf_law_dr_run with stages = 1, per iteration, and its ratio to `solve`
  stages2   rsf_law_dr_run with stages = 2, per iteration and per EXECUTED solve per chain (n_solves from the counters), the latter's
            ratio to `solve`
  fused     Engine.law_dr, the whole call (the start's solve included), per iteration
  split     Engine.dr_from_ssq on law_ssq_fn, the whole call (the start's solve included), per iteration: the path the fused kernel
            replaces, with its two proposals, two solves and two decisions per iteration as launches of their own and the host
            round trip between them; speed_up = split / fused on the same arguments
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import bayesian_markov_chain_monte_carlo_amd as pkg  # noqa: E402

TRUTH = np.array([20.0, 0.011, 0.014])
BOX = {1: (np.array([5.0]), np.array([200.0])), 3: (np.array([8.0, 0.009, 0.012]), np.array([60.0, 0.013, 0.016]))}
K = 4


def step_history(t):
    t = np.asarray(t, dtype=np.float64)
    return np.where((t >= 10.0) & (t < 30.0), 10.0, 1.0)


def stat(ts, per=1.0):
    ts = np.asarray(ts) / per
    return {"median_s": float(np.median(ts)), "min_s": float(ts.min()), "max_s": float(ts.max())}


def one(eng, law, d, n, rounds):
    import torch

    lo, hi = BOX[d]
    truth = TRUTH[:d]
    ab = (None, None) if d == 1 else ([TRUTH[1]], [TRUTH[2]])
    clean = np.asarray(eng.law_observe(law, "mu", [TRUTH[0]], *ab)[1].cpu())[:, 0]
    data = clean + 0.05 * np.abs(clean - clean[0]).max() * np.random.default_rng(1).standard_normal(clean.size)
    L = eng.law_gn_factor(law, "mu", truth, data)[0]
    rng = np.random.default_rng(7)
    q0 = np.ascontiguousarray(truth * (1.0 + 1e-3 * rng.standard_normal((n, d))))
    warm = eng.law_dr(law, "mu", q0, data, lo, hi, L, 16, gamma=0.2, seed=3, keep=0)
    q_host, l_host = warm.q.copy(), warm.l.copy()
    dev = lambda x: eng._in(x)
    q, l, obs = dev(q_host), dev(l_host), dev(data)
    cols = [q[:, p].contiguous() for p in range(d)] + [None] * (3 - d)
    counters = [eng._ints(np.zeros(n)) for _ in range(5)]
    state = {"iter0": 17}

    def run(stages):
        for c in counters:
            c.zero_()
        eng.law_dr_run(law, "mu", q, l, obs, lo, hi, L, K, counters, gamma=0.2, stages=stages, seed=3, iter0=state["iter0"])
        state["iter0"] += K

    calls = {
        "solve": lambda: eng.law_observe(law, "mu", cols[0], cols[1], cols[2], data=obs, want_ssq=True, want_series=False),
        "stages1": lambda: run(1),
        "stages2": lambda: run(2),
        "fused": lambda: eng.law_dr(law, "mu", q_host, data, lo, hi, L, K, gamma=0.2, seed=3, iters_per_launch=K, keep=0, iter0=17),
        "split": lambda: eng.dr_from_ssq(eng.law_ssq_fn(law, data, "mu"), q_host, lo, hi, L, K, 0.5 * eng.nout, gamma=0.2, seed=3, keep=0, iter0=17),
    }
    times, solves, first = {k: [] for k in calls}, [], {}
    for r in range(rounds + 1):  # the first round is the warm-up
        for k, f in calls.items():  # in turn, so that a drift of the machine touches all alike
            eng.sync()
            t = time.perf_counter()
            res = f()
            eng.sync()
            if r:
                times[k].append(time.perf_counter() - t)
            if k == "stages2" and r:
                a1, a2, o1, o2, st = (int(c.sum().item()) for c in counters)
                solves.append(((K * n - st - o1) + (K * n - st - a1 - o2)) / (K * n))
            if k in ("fused", "split") and not r:
                first[k] = res  # the same run by both paths: the same bits
    torch.cuda.synchronize()
    same = all(bool(np.array_equal(getattr(first["fused"], k).view(np.int64), getattr(first["split"], k).view(np.int64))) for k in ("q", "l"))
    out = {"law": law, "d": d, "n": n, "iterations_per_call": K, "fused_is_split_bit_for_bit": same,
           "warm_up_accept_rates": [float(x) for x in warm.accept_rates],
           "solve": stat(times["solve"]), "stages1": stat(times["stages1"], K), "stages2": stat(times["stages2"], K),
           "fused": stat(times["fused"], K), "split": stat(times["split"], K)}
    base = out["solve"]["median_s"]
    spc = float(np.median(solves))
    out["solve_spread"] = out["solve"]["max_s"] / out["solve"]["min_s"] - 1.0
    out["stages1"]["over_solve"] = out["stages1"]["median_s"] / base
    out["stages2"]["solves_per_chain_iteration"] = spc
    out["stages2"]["per_solve_s"] = out["stages2"]["median_s"] / spc
    out["stages2"]["per_solve_over_solve"] = out["stages2"]["median_s"] / spc / base
    out["speed_up"] = out["split"]["median_s"] / out["fused"]["median_s"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="4096 and 256 chains, nsteps 500")
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    sizes, nsteps = ((4096, 256), 500) if args.quick else ((65536, 256), 2000)
    lib = pkg._abi.load()
    import torch

    out = {"device": None, "build_id": lib.rsf_build_id().decode(), "nsteps": nsteps, "rounds": args.rounds, "runs": []}
    with pkg.Engine(mem="device") as eng:
        out["device"] = torch.cuda.get_device_name(eng.device)
        model = pkg.RateStateModel(number_time_steps=nsteps)
        model.loading = step_history
        eng.set_model(model, 1)
        for n in sizes:
            for law in ("aging", "slip"):
                for d in (1, 3):
                    res = one(eng, law, d, n, args.rounds)
                    out["runs"].append(res)
                    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
