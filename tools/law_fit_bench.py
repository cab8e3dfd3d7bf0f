#!/usr/bin/env python3
"""
Cost of the fused Levenberg-Marquardt fit under a state law (include/rsf_law_fit.h) on the GPU, against its own bare solve, against
the split path and against the route it replaces: recorded, not gated.
    python tools/law_fit_bench.py [--out profiles/law_fit/law_fit_bench.json] [--quick]
tools/law_dr_bench.py's method: one process, device-memory engine, every call warmed up (round 0), then the calls timed in turn,
`rounds` times over, each timing a host clock (time.perf_counter) around one call that ends in a device synchronise; a call's state is
put back before its clock starts.  Reported: the median over the rounds with its spread (min, max).  Shape: `starts` starts (65 536,
and 256 where launches and copies dominate) at nsteps 2000 under the step history, friction data of the truth (Dc, a, b) =
(20, 0.011, 0.014) with noise 5 % of the excursion, d = 1 and d = 3, both laws; the starts lie in a ball of 1 % around the truth and
ftol is 0, so that every start is RUNNING through every timed iteration.  Timed, K = 4 iterations per call:
  solve      rsf_law_observe in SSq mode on the (d + 1) n points of the starts and their forward-difference neighbours: the bare solve
  normal     rsf_law_fit_normal, and its ratio to `solve`
  fused      rsf_law_fit_run with n_iter = K, per iteration, and its ratio to `solve`
  split      K times rsf_fit_trial -> rsf_law_fit_normal -> rsf_fit_decide on device memory, per iteration; over_fused = split / fused
  residuals  Engine.fit_from_residuals around law_observe (max_iter = K), the whole call per normal-equation evaluation (K + 1 of them):
             the only route before this family, the series of every point to the host and the normal equations formed there;
             `law_fit` is Engine.law_fit on the same arguments, per evaluation too, and speed_up = residuals / law_fit.  Run up to
             4096 starts only: at 65 536 the residual array alone is 2 to 4 GB on the host.
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
FD = {1: 1e-6, 3: 1e-4}
K = 4
RESIDUALS_MAX = 4096
FIELDS = ("q", "ssq", "grad", "jtj", "lam", "status", "iters")


def step_history(t):
    t = np.asarray(t, dtype=np.float64)
    return np.where((t >= 10.0) & (t < 30.0), 10.0, 1.0)


def stat(ts, per=1.0):
    ts = np.asarray(ts) / per
    return {"median_s": float(np.median(ts)), "min_s": float(ts.min()), "max_s": float(ts.max())}


def one(eng, law, d, n, rounds):
    import torch

    lo, hi = BOX[d]
    fd = FD[d]
    ab = (None, None) if d == 1 else ([TRUTH[1]], [TRUTH[2]])
    clean = np.asarray(eng.law_observe(law, "mu", [TRUTH[0]], *ab)[1].cpu())[:, 0]
    data = clean + 0.05 * np.abs(clean - clean[0]).max() * np.random.default_rng(1).standard_normal(clean.size)
    q_host = np.ascontiguousarray(TRUTH[:d] * (1.0 + 1e-2 * np.random.default_rng(7).uniform(-1.0, 1.0, (n, d))))
    obs = eng._in(data)
    # the (d + 1) n points the group solve integrates, as columns for law_observe
    pq = np.repeat(q_host[None], d + 1, axis=0)
    for p in range(d):
        pq[p + 1, :, p] *= 1 + fd
    pts = eng._in(np.ascontiguousarray(pq.reshape(-1, d)))
    cols = [pts[:, p].contiguous() for p in range(d)] + [None] * (3 - d)
    q = eng._in(q_host)
    ssq, grad, jtj = eng.law_fit_normal(law, "mu", q, obs, fd)
    start = dict(q=q, ssq=ssq, grad=grad, jtj=jtj, lam=eng._in(np.full(n, 1e-3)), status=eng._ints(np.zeros(n)), iters=eng._ints(np.zeros(n)))
    assert bool(torch.isfinite(ssq).all())
    work = {k: v.clone() for k, v in start.items()}
    keep = {}

    def reset():
        for k in FIELDS:
            work[k].copy_(start[k])

    def fused():
        eng.law_fit_run(law, "mu", work["q"], obs, lo, hi, work["ssq"], work["grad"], work["jtj"], work["lam"], work["status"], work["iters"], K, fd, 0.0)

    def split():
        for _ in range(K):
            qt, ok = eng.fit_trial(work["q"], work["grad"], work["jtj"], work["lam"], work["status"], lo, hi)
            s_n, g_n, h_n = eng.law_fit_normal(law, "mu", qt, obs, fd)
            eng.fit_decide(work["q"], work["ssq"], work["grad"], work["jtj"], work["lam"], work["status"], work["iters"], qt, ok, s_n, g_n, h_n, 0.0)

    def res_fn(points):
        points = np.asarray(points, dtype=np.float64)
        c = [np.ascontiguousarray(points[:, p]) for p in range(d)] + [None] * (3 - d)
        s = eng.law_observe(law, "mu", c[0], c[1], c[2], want_series=True)[1]
        return np.asarray(s.cpu()).T - data[None, :]

    calls = {
        "solve": (None, lambda: eng.law_observe(law, "mu", cols[0], cols[1], cols[2], data=obs, want_ssq=True, want_series=False)),
        "normal": (None, lambda: eng.law_fit_normal(law, "mu", q, obs, fd)),
        "fused": (reset, fused),
        "split": (reset, split),
    }
    if n <= RESIDUALS_MAX:
        calls["residuals"] = (None, lambda: eng.fit_from_residuals(res_fn, q_host, lo, hi, fd, 0.0, K))
        calls["law_fit"] = (None, lambda: eng.law_fit(law, "mu", q_host, data, lo, hi, fd, 0.0, K, K))
    times = {k: [] for k in calls}
    for r in range(rounds + 1):  # the first round is the warm-up
        for k, (prep, f) in calls.items():  # in turn, so that a drift of the machine touches all alike
            if prep:
                prep()
            eng.sync()
            t = time.perf_counter()
            res = f()
            eng.sync()
            if r:
                times[k].append(time.perf_counter() - t)
            elif k in ("fused", "split"):
                keep[k] = {x: work[x].clone() for x in FIELDS}  # the same iterations by both paths: the same bits
            elif k in ("residuals", "law_fit"):
                keep[k] = res
    torch.cuda.synchronize()
    bits = lambda x: np.ascontiguousarray(np.asarray(x.cpu())).view(np.int32 if x.element_size() == 4 else np.int64)
    out = {"law": law, "d": d, "n": n, "iterations_per_call": K,
           "fused_is_split_bit_for_bit": all(bool(np.array_equal(bits(keep["fused"][x]), bits(keep["split"][x]))) for x in FIELDS),
           "accepted_per_start": float((keep["fused"]["lam"] < 1e-3).float().mean().item()),
           "solve": stat(times["solve"]), "normal": stat(times["normal"]), "fused": stat(times["fused"], K), "split": stat(times["split"], K)}
    base = out["solve"]["median_s"]
    out["solve_spread"] = out["solve"]["max_s"] / out["solve"]["min_s"] - 1.0
    out["normal"]["over_solve"] = out["normal"]["median_s"] / base
    out["fused"]["over_solve"] = out["fused"]["median_s"] / base
    out["split"]["over_fused"] = out["split"]["median_s"] / out["fused"]["median_s"]
    if "residuals" in calls:
        out["residuals"], out["law_fit"] = stat(times["residuals"], K + 1), stat(times["law_fit"], K + 1)
        out["speed_up"] = out["residuals"]["median_s"] / out["law_fit"]["median_s"]
        a, b = keep["residuals"], keep["law_fit"]
        out["residuals_best_dc"], out["law_fit_best_dc"] = float(a.q[a.best(), 0]), float(b.q[b.best(), 0])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="4096 and 256 starts, nsteps 500")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--laws", default="aging,slip")
    args = ap.parse_args()
    sizes, nsteps = ((4096, 256), 500) if args.quick else ((65536, 4096, 256), 2000)
    lib = pkg._abi.load()
    import torch

    out = {"device": None, "build_id": lib.rsf_build_id().decode(), "nsteps": nsteps, "rounds": args.rounds,
           "clock": "time.perf_counter around one call that ends in a device synchronise", "runs": []}
    with pkg.Engine(mem="device") as eng:
        out["device"] = torch.cuda.get_device_name(eng.device)
        model = pkg.RateStateModel(number_time_steps=nsteps)
        model.loading = step_history
        eng.set_model(model, 1)
        for n in sizes:
            for law in args.laws.split(","):
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
