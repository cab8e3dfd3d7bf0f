#!/usr/bin/env python3
"""
Cost of the fused delayed-rejection sampler with the stiffness among the parameters (include/rsf_kstiff.h) on the GPU, against the
kernel with a constant stiffness whose loop it restates: recorded, not gated.
    python tools/kstiff_bench.py [--out profiles/kstiff/kstiff_bench.json] [--quick]
tools/stiff_bench.py's method: one process, device-memory engine, every call warmed up, then the calls timed in turn, `rounds`
times over, each timing a host clock around one call that ends in a device synchronise; reported: the median over the rounds
with its spread (min, max).  Shape: `chains` chains (65 536 and 256) at nsteps 2000 under the step history, friction data of the
truth (Dc, a, b, k) = (20, 0.011, 0.014, 2e-3) with noise 5 % of the excursion, the ageing law, one and two stages.  Each kernel
runs on a sample of its own target (16 iterations of its sampler from a ball around the truth) with its own Gauss-Newton factor at the
truth: stiff_dr over Dc (d = 1) or (Dc, a, b) (d = 3) at the true stiffness, kstiff_dr over (Dc, k) (d = 2) or (Dc, a, b, k) (d = 4).
Both spend one solve per stage; what a wave spends also depends on how many of its lanes propose inside the box, which the
counters report (solves_per_iteration).
Timed, K = 4 iterations per call, pairs (stiff d = 1, kstiff d = 2) and (stiff d = 3, kstiff d = 4):
  stiff_dr   rsf_stiff_dr_run (stiff_dr_kernel), per iteration — timed TWICE per round (stiff_dr, stiff_dr_again): the ratio of the two
             is the spread of the kernel against itself, what a ratio between kernels is read beside
  kstiff_dr  rsf_kstiff_dr_run (kstiff_dr_kernel), per iteration; over_stiff_dr = kstiff_dr / stiff_dr
  fused      Engine.kstiff_dr continuing the sample (l0 given: no start's solve), the whole call, per iteration
  split      rsf_kstiff_dr_propose -> rsf_kstiff_observe -> rsf_kstiff_dr_accept stage by stage, with the host round trip between
             them, per iteration; speed_up = split / fused on the same arguments
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
STIFFNESS = 2e-3
BOX = {1: (np.array([5.0]), np.array([200.0])), 3: (np.array([8.0, 0.009, 0.012]), np.array([60.0, 0.013, 0.016]))}
K_BOX = (5e-4, 8e-3)
K = 4


def step_history(t):
    t = np.asarray(t, dtype=np.float64)
    return np.where((t >= 10.0) & (t < 30.0), 10.0, 1.0)


def stat(ts, per=1.0):
    ts = np.asarray(ts) / per
    return {"median_s": float(np.median(ts)), "min_s": float(ts.min()), "max_s": float(ts.max())}


def solves(counters, n, stages):
    """forward solves per chain and iteration of a K-iteration call, from its counters (DrResult.n_solves' rule)"""
    a1, a2, o1, o2, stuck = (int(c.sum().item()) for c in counters)
    first = K * n - stuck - o1
    return (first + ((K * n - stuck - a1 - o2) if stages == 2 else 0)) / (K * n)


def one(eng, d, n, rounds, law="aging"):
    """the pair (stiff_dr at d, kstiff_dr at d + 1) on n chains"""
    lo, hi = BOX[d]
    klo, khi = np.append(lo, K_BOX[0]), np.append(hi, K_BOX[1])
    truth, ktruth = TRUTH[:d], np.append(TRUTH[:d], STIFFNESS)
    ab = (None, None) if d == 1 else ([TRUTH[1]], [TRUTH[2]])
    clean = np.asarray(eng.stiff_observe(law, "mu", STIFFNESS, [TRUTH[0]], *ab)[1].cpu())[:, 0]
    data = clean + 0.05 * np.abs(clean - clean[0]).max() * np.random.default_rng(1).standard_normal(clean.size)
    L = eng.law_gn_factor(law, "mu", truth, data, stiffness=STIFFNESS)[0]
    kL = eng.kstiff_gn_factor(law, "mu", ktruth, data)[0]
    rng = np.random.default_rng(7)
    ball = 1.0 + 1e-3 * rng.standard_normal((n, d + 1))
    warm = eng.law_dr(law, "mu", np.ascontiguousarray(truth * ball[:, :d]), data, lo, hi, L, 16, gamma=0.2, seed=3, keep=0, stiffness=STIFFNESS)
    kwarm = eng.kstiff_dr(law, "mu", np.ascontiguousarray(ktruth * ball), data, klo, khi, kL, 16, gamma=0.2, seed=3, keep=0)
    state = {"stiff": (warm.q.copy(), warm.l.copy()), "kstiff": (kwarm.q.copy(), kwarm.l.copy())}
    obs = eng._in(data)
    counters = [eng._ints(np.zeros(n)) for _ in range(5)]

    def run(stages, which):
        # every timed call starts from the same chains at the same Philox iterations
        q, l = (eng._in(x) for x in state[which])
        for c in counters:
            c.zero_()
        eng.sync()
        t = time.perf_counter()
        if which == "stiff":
            eng.stiff_dr_run(law, "mu", STIFFNESS, q, l, obs, lo, hi, L, K, counters, gamma=0.2, stages=stages, seed=3, iter0=17)
        else:
            eng.kstiff_dr_run(law, "mu", q, l, obs, klo, khi, kL, K, counters, gamma=0.2, stages=stages, seed=3, iter0=17)
        eng.sync()
        return time.perf_counter() - t, solves(counters, n, stages)

    def whole(f):
        eng.sync()
        t = time.perf_counter()
        res = f()
        eng.sync()
        return time.perf_counter() - t, res

    out = {"law": law, "d_stiff": d, "d_kstiff": d + 1, "n": n, "iterations_per_call": K, "stiffness": STIFFNESS,
           "warm_up_accept_rates": {"stiff": [float(x) for x in warm.accept_rates], "kstiff": [float(x) for x in kwarm.accept_rates]}}
    for stages in (1, 2):
        calls = {"stiff_dr": lambda: run(stages, "stiff"), "kstiff_dr": lambda: run(stages, "kstiff"), "stiff_dr_again": lambda: run(stages, "stiff")}
        times, spent = {k: [] for k in calls}, {}
        for r in range(rounds + 1):  # the first round is the warm-up
            for k, f in calls.items():  # in turn, so that a drift of the machine touches all alike
                t, spent[k] = f()
                if r:
                    times[k].append(t)
        res = {k: stat(v, K) for k, v in times.items()}
        res["solves_per_iteration"] = {k: spent[k] for k in ("stiff_dr", "kstiff_dr")}
        res["over_stiff_dr"] = res["kstiff_dr"]["median_s"] / res["stiff_dr"]["median_s"]
        res["stiff_dr_against_itself"] = res["stiff_dr_again"]["median_s"] / res["stiff_dr"]["median_s"]
        res["stiff_dr_spread"] = res["stiff_dr"]["max_s"] / res["stiff_dr"]["min_s"] - 1.0
        out[f"stages{stages}"] = res

    q_host, l_host = state["kstiff"]

    def split():
        q, l, cnt = q_host.copy(), l_host.copy(), [np.zeros(n, dtype=np.int32) for _ in range(5)]
        fn = host.kstiff_ssq_fn(law, data, "mu")
        shape = 0.5 * host.nout

        def solved(y, mask):
            s, inside = np.ones(n), np.asarray(mask).astype(bool)
            if inside.any():
                s[inside] = fn(np.asarray(y)[inside])
            return s

        for k in range(K):
            kw = dict(gamma=0.2, seed=3, offset=0, iteration=17 + k)
            y, mask = host.kstiff_dr_propose(q, l, klo, khi, kL, 1, **kw)
            l1, pend = host.kstiff_dr_accept(q, l, klo, khi, 1, y, mask, solved(y, mask), cnt, shape, **kw)
            y, mask = host.kstiff_dr_propose(q, l, klo, khi, kL, 2, pending=pend, **kw)
            host.kstiff_dr_accept(q, l, klo, khi, 2, y, mask, solved(y, mask), cnt, shape, l1=l1, pending=pend, **kw)
        return q, l

    def fused():
        res = eng.kstiff_dr(law, "mu", q_host, data, klo, khi, kL, K, gamma=0.2, seed=3, iters_per_launch=K, keep=0, iter0=17, l0=l_host)
        return res.q, res.l

    with pkg.Engine(mem="host") as host:  # the split path's calls take host arrays
        host.set_model(*eng.model_args)
        calls = {"fused": fused, "split": split}
        times, first = {k: [] for k in calls}, {}
        for r in range(rounds + 1):
            for k, f in calls.items():
                t, res = whole(f)
                if r:
                    times[k].append(t)
                else:
                    first[k] = res  # the same run by both paths: the same bits
    out["fused_is_split_bit_for_bit"] = all(bool(np.array_equal(a.view(np.int64), b.view(np.int64))) for a, b in zip(first["fused"], first["split"]))
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
        eng.set_model(model, 1)  # no stiffness of the model's: both kernels run on one engine, the calls name it or carry it
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
