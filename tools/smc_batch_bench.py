#!/usr/bin/env python3
"""
Cost of the batched SMC populations (include/rsf_smc_batch.h) against the sequential loop they replace: one process,
device-memory engine, median of 5 after a warm-up.
    python tools/smc_batch_bench.py [--out profiles/smc/smc_batch_bench.json] [--quick] [--trace]
  move     rsf_smc_batch_move at P = 8, n = 4096, nsteps 2000, d = 1 and 3 (3 steps) against eight sequential rsf_smc_move calls on
           the same populations, and against the bare rsf_forward_batch SSq solve of 8 x 4096 lanes, once per step
  whole    Engine.smc_batch with 8 replicates (d = 1, nsteps 500, n = 4096, the box (0, 1e4)) against eight sequential Engine.smc runs
  --trace  one batched move, one sequential loop and one whole run of each kind and nothing else, for a
           `rocprofv3 --kernel-trace --stats -- python tools/smc_batch_bench.py --trace` run of its own
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

P, N, STEPS = 8, 4096, 3
BOX = {1: ([600.0], [1600.0]), 3: ([850.0, 0.009, 0.0145], [1150.0, 0.013, 0.0158])}
STEP = {1: np.diag([3.0]), 3: np.diag([3.0, 2e-5, 2e-5])}  # a small step: nearly every proposal is inside the box and is solved


def median_time(fn, sync, reps=5):
    fn()
    sync()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        sync()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)), [float(t) for t in ts]


def observation(eng, model, dc=1000.0):
    eng.set_model(model, 1)
    truth = np.asarray(eng.forward([dc])[1].cpu())[:, 0]
    return truth + 0.01 * np.abs(truth).max() * np.random.default_rng(1).standard_normal(truth.size)


def move_case(eng, d, nsteps):
    import torch

    model = pkg.RateStateModel(number_time_steps=nsteps)
    data = torch.as_tensor(observation(eng, model), device=f"cuda:{eng.device}").reshape(1, -1)
    lo, hi = BOX[d]
    seeds = np.arange(1, P + 1)
    q = eng.smc_batch_init(lo, hi, N, seeds)
    l = eng.smc_batch_logtarget(q, data, 0, lo, hi)
    chol = np.tile(STEP[d], (P, 1, 1))
    batch = lambda: eng.smc_batch_move(q, l, data, 0, lo, hi, chol, 0.5, seeds, 0, 1, STEPS, inplace=False)
    loop = lambda: [eng.smc_move(q[p], l[p], data[0], lo, hi, chol[p], 0.5, int(seeds[p]), 0, 1, STEPS) for p in range(P)]
    flat = q.reshape(P * N, d)
    cols = [flat[:, k].contiguous() for k in range(d)]
    bare = lambda: eng.forward(cols[0], a=cols[1] if d == 3 else None, b=cols[2] if d == 3 else None, data=data[0], want_ssq=True, want_acc=False)
    return batch, loop, bare


def bench_move(eng, d, nsteps):
    batch, loop, bare = move_case(eng, d, nsteps)
    t0, _ = median_time(bare, eng.sync)
    tl, rl = median_time(loop, eng.sync)
    tb, rb = median_time(batch, eng.sync)
    t1, _ = median_time(bare, eng.sync)
    return {"d": d, "P": P, "n": N, "nsteps": nsteps, "steps": STEPS, "bare_solve_s": [t0, t1], "sequential_s": tl, "sequential_runs_s": rl,
            "batched_s": tb, "batched_runs_s": rb, "batched_over_sequential": tb / tl, "batched_per_step_over_bare": tb / STEPS / (0.5 * (t0 + t1))}


def whole_case(eng, nsteps=500):
    model = pkg.RateStateModel(number_time_steps=nsteps)
    data = observation(eng, model)
    batch = lambda: eng.smc_batch(data, [0.0], [1.0e4], N, replicates=P)
    loop = lambda: [eng.smc(data, [0.0], [1.0e4], N, seed=s) for s in range(P)]
    return batch, loop


def bench_whole(eng):
    batch, loop = whole_case(eng)
    tl, rl = median_time(loop, eng.sync)
    tb, rb = median_time(batch, eng.sync)
    out, singles = batch(), loop()
    same = all(r["log_evidence"] == s["log_evidence"] for r, s in zip(out["runs"], singles))
    return {"d": 1, "replicates": P, "n": N, "nsteps": 500, "sequential_s": tl, "sequential_runs_s": rl, "batched_s": tb, "batched_runs_s": rb,
            "batched_over_sequential": tb / tl, "stages": [len(r["stages"]) for r in out["runs"]], "same_log_evidence_as_the_loop": same,
            "summary": out["summary"][0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smc", "smc_batch_bench.json"))
    ap.add_argument("--quick", action="store_true", help="nsteps 500 in the move as well")
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    nsteps = 500 if a.quick else 2000
    with pkg.Engine(mem="device") as eng:
        if a.trace:
            for d in (1, 3):
                batch, loop, _ = move_case(eng, d, nsteps)
                batch(), loop(), eng.sync()
            batch, loop = whole_case(eng)
            batch(), loop(), eng.sync()
            return
        res = {"build_id": pkg._abi.load().rsf_build_id().decode(), "move": [], "whole": None}
        for d in (1, 3):
            res["move"].append(bench_move(eng, d, nsteps))
            print(json.dumps(res["move"][-1]), flush=True)
        res["whole"] = bench_whole(eng)
        print(json.dumps(res["whole"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
