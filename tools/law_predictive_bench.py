#!/usr/bin/env python3
"""
Cost of the posterior predictive checks under a state law (include/rsf_law_predict.h) against their bare solve, on the GPU:
recorded, not gated.
    python tools/law_predictive_bench.py [--out profiles/law_predictive/law_predictive_bench.json] [--quick]
tools/observe_bench.py's method: one process, a device-memory engine, every call warmed up, then the calls timed in turn,
`rounds` times over, each timing a host clock around `reps` calls that ends in a device synchronise; reported: the median over
the rounds and the spread (min, max).  Shapes: 65 536 and 262 144 draws at nsteps 2000 under the step history, friction data,
d = 1 and 3, both laws; the draws uniform in [15, 25] x [0.0105, 0.0115] x [0.0135, 0.0145].  Per shape:
    solve           rsf_law_observe, SSq only: the bare solve
    fused           rsf_law_predict_partials without the series
    fused_series    rsf_law_predict_partials with the series
    split           rsf_law_observe with the series, then rsf_predict_series_partials
    series_partials rsf_predict_series_partials alone, with the bytes it reads over its time
and the ratios fused / solve (the yardstick: rsf_predict_partials over its own solve, 2.8 to 3.0), fused_series /
solve and split / solve.  Before any timing the fused partials are compared with the split path's bit for bit.
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


def step_history(t):
    """a velocity step (tests/law_reference.py's step_history): V_l = 1, then 10 on [10, 30), then 1"""
    t = np.asarray(t, dtype=np.float64)
    return np.where((t >= 10.0) & (t < 30.0), 10.0, 1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="4096 draws, nsteps 500, three rounds")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=4, help="calls per timed window")
    args = ap.parse_args()
    sizes, nsteps, rounds = ((4096,), 500, 3) if args.quick else ((65536, 262144), 2000, args.rounds)
    lib = pkg._abi.load()
    import torch

    out = {"device": None, "build_id": lib.rsf_build_id().decode(), "nsteps": nsteps, "rounds": rounds, "reps": args.reps, "history": "step",
           "observable": "mu", "cases": []}
    with pkg.Engine(mem="device") as eng:
        out["device"] = torch.cuda.get_device_name(eng.device)
        for law in ("aging", "slip"):
            model = pkg.RateStateModel(number_time_steps=nsteps)
            model.loading, model.state_law, model.observable = step_history, law, "mu"
            eng.set_model(model, 1)
            truth = np.asarray(eng.law_observe(law, "mu", [20.0])[1].cpu())[:, 0]
            amp = np.abs(truth - truth[0]).max()
            data = eng._in(truth + 0.05 * amp * np.random.default_rng(1).standard_normal(truth.size))
            cy = truth.copy()
            for d in (1, 3):
                for n in sizes:
                    rng = np.random.default_rng([2, d, n])
                    qh = np.column_stack([rng.uniform(15.0, 25.0, n), rng.uniform(0.0105, 0.0115, n), rng.uniform(0.0135, 0.0145, n)])[:, :d]
                    s2h = (rng.uniform(0.05, 0.2, n) * amp) ** 2
                    cl = -0.5 * np.log(2.0 * np.pi * s2h.mean()) - (np.asarray(data.cpu()) - cy) ** 2 / (2.0 * s2h.mean())
                    q, s2 = eng._in(np.ascontiguousarray(qh)), eng._in(s2h)
                    dc = q[:, 0].contiguous()
                    ab = [q[:, p].contiguous() for p in (1, 2)] if d == 3 else [None, None]
                    series = eng.law_observe(law, "mu", dc, ab[0], ab[1])[1]
                    calls = {
                        "solve": lambda: eng.law_observe(law, "mu", dc, ab[0], ab[1], data=data, want_ssq=True, want_series=False)[0],
                        "fused": lambda: eng.law_predictive_partials(law, "mu", q, s2, data, cy, cl),
                        "fused_series": lambda: eng.law_predictive_partials(law, "mu", q, s2, data, cy, cl, return_series=True)[0],
                        "split": lambda: eng.series_partials(eng.law_observe(law, "mu", dc, ab[0], ab[1])[1], s2, data, cy, cl),
                        "series_partials": lambda: eng.series_partials(series, s2, data, cy, cl),
                    }
                    res = {k: f() for k, f in calls.items()}  # the warm-up of every call timed, and the results
                    eng.sync()
                    case = {"law": law, "d": d, "n": n,
                            "fused_is_split_bit_for_bit": bool(all(np.array_equal(res["fused"].view(np.int64), res[k].view(np.int64))
                                                                   for k in ("fused_series", "split", "series_partials"))),
                            "all_finite": bool(np.isfinite(res["fused"]).all() and torch.isfinite(res["solve"]).all().item())}
                    times = {k: [] for k in calls}
                    for _ in range(rounds):
                        for k, f in calls.items():  # in turn, so that a drift of the machine touches all alike
                            eng.sync()
                            t = time.perf_counter()
                            for _ in range(args.reps):
                                f()
                            eng.sync()
                            times[k].append((time.perf_counter() - t) / args.reps)
                    for k, ts in times.items():
                        case[k] = {"median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts))}
                    base = case["solve"]["median_s"]
                    case["solve"]["ns_per_lane_step"] = base / (n * (eng.nout - 1)) * 1e9
                    case["solve_spread"] = case["solve"]["max_s"] / case["solve"]["min_s"] - 1.0
                    for k in ("fused", "fused_series", "split"):
                        case[k]["over_solve"] = case[k]["median_s"] / base
                    case["series_partials"]["bytes_read"] = 8 * n * eng.nout
                    case["series_partials"]["read_GB_per_s"] = 8 * n * eng.nout / case["series_partials"]["median_s"] / 1e9
                    out["cases"].append(case)
                    del series, res
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
