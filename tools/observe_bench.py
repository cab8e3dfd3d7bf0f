#!/usr/bin/env python3
"""
Cost of the observables of the state-law solve (include/rsf_observe.h, rsf_law_observe) against rsf_law_forward — whose kernel
is the parent's, instruction for instruction (profiles/observe/kernel_diff.log) — on the GPU: recorded, not gated.
    python tools/observe_bench.py [--out profiles/observe/observe_bench.json] [--quick] [--law aging]
One process, device-memory engine, SSq mode (no series), the same 65 536 points (Dc log-uniform over [300, 5000]) at nsteps 2000
under the built-in history.  Every call is warmed up, then the calls are timed in turn, `rounds` times over, each timing a host
clock around `reps` calls that ends in a device synchronise; reported: the median over the rounds, the spread (min, max), each
observable's ratio to rsf_law_forward's median, and rsf_law_forward's own spread max / min - 1, which a ratio has to leave
before it says anything about the kernel.  Before any timing rsf_law_observe's "acc" is compared with rsf_law_forward bit for bit.
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

OBSERVABLES = ("acc", "mu", "theta", "velocity")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="4096 points, nsteps 500")
    ap.add_argument("--law", default="aging")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=16, help="calls per timed window")
    args = ap.parse_args()
    n, nsteps = (4096, 500) if args.quick else (65536, 2000)
    lib = pkg._abi.load()
    out = {"device": None, "build_id": lib.rsf_build_id().decode(), "law": args.law, "n": n, "nsteps": nsteps, "rounds": args.rounds, "reps": args.reps}
    import torch

    with pkg.Engine(mem="device") as eng:
        out["device"] = torch.cuda.get_device_name(eng.device)
        eng.set_model(pkg.RateStateModel(number_time_steps=nsteps), 1)
        dc = eng._in(np.exp(np.random.default_rng(2).uniform(np.log(300.0), np.log(5000.0), n)))
        calls = {}
        for obs in OBSERVABLES:  # each observable against a noisy series of its own
            truth = np.asarray(eng.law_observe(args.law, obs, [1000.0])[1].cpu())[:, 0]
            scale = np.abs(truth - truth[0]).max() or 1.0
            data = eng._in(truth + 0.01 * scale * np.random.default_rng(1).standard_normal(truth.size))
            if obs == "acc":
                calls["law_forward"] = lambda data=data: eng.law_forward(args.law, dc, data=data, want_ssq=True, want_acc=False)[0]
            calls[f"law_observe_{obs}"] = lambda obs=obs, data=data: eng.law_observe(args.law, obs, dc, data=data, want_ssq=True, want_series=False)[0]
        res = {k: np.asarray(f().cpu()) for k, f in calls.items()}  # the warm-up of every call timed, and the results
        eng.sync()
        out["acc_is_law_forward_bit_for_bit"] = bool(np.array_equal(res["law_forward"].view(np.int64), res["law_observe_acc"].view(np.int64)))
        out["all_finite"] = bool(all(np.isfinite(v).all() for v in res.values()))
        times = {k: [] for k in calls}
        for _ in range(args.rounds):
            for k, f in calls.items():  # in turn, so that a drift of the machine touches all alike
                eng.sync()
                t = time.perf_counter()
                for _ in range(args.reps):
                    f()
                eng.sync()
                times[k].append((time.perf_counter() - t) / args.reps)
    steps = n * (nsteps - 1)
    for k, ts in times.items():
        out[k] = {"median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts)), "ns_per_lane_step": float(np.median(ts)) / steps * 1e9}
    base = out["law_forward"]
    out["law_forward_spread"] = base["max_s"] / base["min_s"] - 1.0
    for obs in OBSERVABLES:
        out[f"law_observe_{obs}"]["over_law_forward"] = out[f"law_observe_{obs}"]["median_s"] / base["median_s"]
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
