#!/usr/bin/env python3
"""
Cost of the fused delayed-rejection sampler with a stiffness independent of Dc (include/rsf_stiff.h) on the GPU, against the
coupled kernel it restates and against the split path it replaces: recorded, not gated.
    python tools/stiff_bench.py [--out profiles/stiff/stiff_bench.json] [--quick]
tools/law_dr_bench.py's method: one process, device-memory engine, every call warmed up, then the calls timed in turn, `rounds`
times over, each timing a host clock around one call that ends in a device synchronise; reported: the median over the rounds
with its spread (min, max).  Shape: `chains` chains (65 536 and 256) at nsteps 2000 under the step history, friction data of the
truth (Dc, a, b) = (20, 0.011, 0.014) with noise 5 % of the excursion, d = 1 and d = 3, the ageing law, one and two stages; the
stiffness is 0.1 / 20, the coupling's own value at the truth, so that the chains of both kernels sample about the same target; the
chains are a sample of it (16 iterations of the sampler from a ball around the truth), the factor law_gn_factor's at the truth.
Timed, K = 4 iterations per call:
  law_dr    rsf_law_dr_run (law_dr_kernel), per iteration — timed TWICE per round (law_dr, law_dr_again): the ratio of the two is the
            spread of the kernel against itself, what a ratio between kernels is read beside
  stiff_dr  rsf_stiff_dr_run (stiff_dr_kernel) on the same chains, per iteration; over_law_dr = stiff_dr / law_dr
  fused     Engine.law_dr with the stiffness, the whole call (the start's solve included), per iteration
  split     Engine.dr_from_ssq on law_ssq_fn with the stiffness, the whole call: rsf_dr_propose -> rsf_stiff_observe -> rsf_dr_accept,
            stage by stage, with the host round trip between them; speed_up = split / fused on the same arguments
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
STIFFNESS = 1e-2 * 10 / 20.0


def step_history(t):
    t = np.asarray(t, dtype=np.float64)
    return np.where((t >= 10.0) & (t < 30.0), 10.0, 1.0)


def stat(ts, per=1.0):
    ts = np.asarray(ts) / per
    return {"median_s": float(np.median(ts)), "min_s": float(ts.min()), "max_s": float(ts.max())}


def one(eng, d, n, rounds, law="aging"):
    import torch

    lo, hi = BOX[d]
    truth = TRUTH[:d]
    ab = (None, None) if d == 1 else ([TRUTH[1]], [TRUTH[2]])
    clean = np.asarray(eng.stiff_observe(law, "mu", STIFFNESS, [TRUTH[0]], *ab)[1].cpu())[:, 0]
    data = clean + 0.05 * np.abs(clean - clean[0]).max() * np.random.default_rng(1).standard_normal(clean.size)
    L = eng.law_gn_factor(law, "mu", truth, data, stiffness=STIFFNESS)[0]
    rng = np.random.default_rng(7)
    q0 = np.ascontiguousarray(truth * (1.0 + 1e-3 * rng.standard_normal((n, d))))
    warm = eng.law_dr(law, "mu", q0, data, lo, hi, L, 16, gamma=0.2, seed=3, keep=0, stiffness=STIFFNESS)
    q_host, l_host = warm.q.copy(), warm.l.copy()
    obs = eng._in(data)
    counters = [eng._ints(np.zeros(n)) for _ in range(5)]

    def run(stages, stiffness):
        # every timed call starts from the same chains at the same Philox iterations: the same proposals for both kernels
        q, l = eng._in(q_host), eng._in(l_host)
        for c in counters:
            c.zero_()
        eng.sync()
        t = time.perf_counter()
        if stiffness is None:
            eng.law_dr_run(law, "mu", q, l, obs, lo, hi, L, K, counters, gamma=0.2, stages=stages, seed=3, iter0=17)
        else:
            eng.stiff_dr_run(law, "mu", stiffness, q, l, obs, lo, hi, L, K, counters, gamma=0.2, stages=stages, seed=3, iter0=17)
        eng.sync()
        return time.perf_counter() - t

    def whole(f):
        eng.sync()
        t = time.perf_counter()
        res = f()
        eng.sync()
        return time.perf_counter() - t, res

    out = {"law": law, "d": d, "n": n, "iterations_per_call": K, "stiffness": STIFFNESS, "warm_up_accept_rates": [float(x) for x in warm.accept_rates]}
    for stages in (1, 2):
        calls = {"law_dr": lambda: run(stages, None), "stiff_dr": lambda: run(stages, STIFFNESS), "law_dr_again": lambda: run(stages, None)}
        times = {k: [] for k in calls}
        for r in range(rounds + 1):  # the first round is the warm-up
            for k, f in calls.items():  # in turn, so that a drift of the machine touches all alike
                t = f()
                if r:
                    times[k].append(t)
        res = {k: stat(v, K) for k, v in times.items()}
        res["over_law_dr"] = res["stiff_dr"]["median_s"] / res["law_dr"]["median_s"]
        res["law_dr_against_itself"] = res["law_dr_again"]["median_s"] / res["law_dr"]["median_s"]
        res["law_dr_spread"] = res["law_dr"]["max_s"] / res["law_dr"]["min_s"] - 1.0
        out[f"stages{stages}"] = res
    calls = {
        "fused": lambda: eng.law_dr(law, "mu", q_host, data, lo, hi, L, K, gamma=0.2, seed=3, iters_per_launch=K, keep=0, iter0=17, stiffness=STIFFNESS),
        "split": lambda: eng.dr_from_ssq(eng.law_ssq_fn(law, data, "mu", stiffness=STIFFNESS), q_host, lo, hi, L, K, 0.5 * eng.nout, gamma=0.2, seed=3,
                                         keep=0, iter0=17),
    }
    times, first = {k: [] for k in calls}, {}
    for r in range(rounds + 1):
        for k, f in calls.items():
            t, res = whole(f)
            if r:
                times[k].append(t)
            else:
                first[k] = res  # the same run by both paths: the same bits
    torch.cuda.synchronize()
    out["fused_is_split_bit_for_bit"] = all(bool(np.array_equal(getattr(first["fused"], k).view(np.int64), getattr(first["split"], k).view(np.int64)))
                                            for k in ("q", "l"))
    out["fused"], out["split"] = stat(times["fused"], K), stat(times["split"], K)
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
        eng.set_model(model, 1)  # no stiffness of the model's: the coupled kernel and the new one run on one engine, the calls name it
        for n in sizes:
            for d in (1, 3):
                res = one(eng, d, n, args.rounds)
                out["runs"].append(res)
                print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
