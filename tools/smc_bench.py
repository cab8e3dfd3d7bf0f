#!/usr/bin/env python3
"""
Cost of the tempered SMC sampler (include/rsf_smc.h) on the GPU: one process, device-memory engine, median of 5 after a warm-up.
    python tools/smc_bench.py [--out profiles/smc/smc_bench.json] [--quick]
  move     rsf_smc_move per Metropolis step against rsf_forward_batch with ssq_out only at the same (n, nsteps), the bare solve
           timed before and after in the same process
  stage    weight sums (16 candidates), resampling (scan, ancestors, gather) against the bytes they must move at 6.3 TB/s
  whole    Engine.smc on the d = 3 problem of DESIGN.md 4g (nsteps 500, 1 % noise) against sample_batched (4096 x 400) plus
           PosteriorPool.evidence on the same data: wall time, forward solves, log evidence and its spread over 8 seeds
    python tools/smc_bench.py --spec-sd     (CPU only) the spread of the specification's log I on the real d = 1 problem of
           tests/test_gpu_smc.py over 32 seeds: the constant SPEC_SD_REAL of tests/smc_cases.py
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import bayesian_markov_chain_monte_carlo_amd as pkg  # noqa: E402

HBM = 6.3e12  # bytes / s
BOX3 = ([850.0, 0.009, 0.0145], [1150.0, 0.013, 0.0158])


def median_time(fn, sync, reps=5):
    fn()
    sync()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        sync()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts))


def observation(eng, model, d):
    eng.set_model(model, 1)
    truth = np.asarray(eng.forward([1000.0])[1].cpu())[:, 0]
    return truth + 0.01 * np.abs(truth).max() * np.random.default_rng(1).standard_normal(truth.size)


def bench_move(eng, n, nsteps, d=3, steps=3):
    import torch

    model = pkg.RateStateModel(number_time_steps=nsteps)
    data = observation(eng, model, d)
    lo, hi = BOX3
    q = eng.smc_init(lo, hi, n, 1)
    l = eng.evidence_logtarget(q, data, lo, hi, torch.zeros(n, dtype=torch.float64, device=q.device))
    chol = np.diag([3.0, 2e-5, 2e-5])  # a small step: nearly every proposal is inside the box and is solved
    dt = torch.as_tensor(data, device=q.device)
    bare = lambda: eng.forward(q[:, 0].contiguous(), a=q[:, 1].contiguous(), b=q[:, 2].contiguous(), data=dt, want_ssq=True, want_acc=False)
    t0 = median_time(bare, eng.sync)
    tm = median_time(lambda: eng.smc_move(q, l, dt, lo, hi, chol, 0.5, 1, 0, 1, steps), eng.sync) / steps
    t1 = median_time(bare, eng.sync)
    return {"n": n, "nsteps": nsteps, "bare_solve_s": [t0, t1], "move_per_step_s": tm, "ratio": tm / (0.5 * (t0 + t1))}


def bench_stage(eng, n, d=3):
    import torch

    g = torch.Generator(device="cuda").manual_seed(1)
    l = -40.0 + 2.0 * torch.randn(n, dtype=torch.float64, device="cuda", generator=g)
    q = torch.rand((n, d), dtype=torch.float64, device="cuda", generator=g)
    cand = [k / 16 for k in range(1, 17)]
    tw = median_time(lambda: eng.smc_weight_sums(l, cand), eng.sync)
    tr = median_time(lambda: eng.smc_resample(q, l, 0.5, -30.0, 0.37), eng.sync)
    bw = 2 * 8 * n  # l read by the max pass and by the sums
    br = 8 * n * (2 + 1 + 1 + 1 + 2 * d + 2)  # l twice, cum out, cum searched, anc out and in, q and l gathered
    return {"n": n, "weight_sums_s": tw, "weight_sums_floor_s": bw / HBM, "resample_s": tr, "resample_floor_s": br / HBM}


def bench_whole(seeds=8):
    model = pkg.RateStateModel(number_time_steps=500)
    lo, hi = BOX3
    out = {"smc": [], "mcmc": []}
    with pkg.Engine(mem="device") as eng:
        data = observation(eng, model, 3)
        for s in range(seeds):
            t = time.perf_counter()
            r = eng.smc(data, lo, hi, 16384, seed=s)
            eng.sync()
            out["smc"].append({"seed": s, "wall_s": time.perf_counter() - t, "solves": r["n_solves"], "log_evidence": r["log_evidence"],
                               "stages": len(r["stages"]), "accept": [round(x["accept_rate"], 3) for x in r["stages"]]})
    m = pkg.MCMC(model, data, 1000.0, [["Uniform", l_, h_] for l_, h_ in zip(lo, hi)], [1000.0, model.a, model.b], nsamples=400, verbose=False)
    m.n0 = 0.0
    for s in range(seeds):
        t = time.perf_counter()
        pool = m.sample_batched(4096, seed=s, n_iters=400)
        ev = pool.evidence(model, data, lo, hi)
        out["mcmc"].append({"seed": s, "wall_s": time.perf_counter() - t, "solves": 4096 * 400 + ev["n1"] + ev["n2"], "log_evidence": ev["log_evidence"],
                            "re": ev["re"]})
    for k in ("smc", "mcmc"):
        v = np.array([x["log_evidence"] for x in out[k]])
        out[k + "_mean"], out[k + "_sd"] = float(v.mean()), float(v.std(ddof=1))
    out["difference"] = out["smc_mean"] - out["mcmc_mean"]
    return out


def spec_sd(seeds=32):
    import posterior_reference as R
    import rsf_oracle
    import smc_reference as ref

    cpu = pkg.Engine(lib=pkg._abi.bind(ctypes.CDLL(rsf_oracle.build())), checker=True, cpu_threads=16)
    model = pkg.RateStateModel(number_time_steps=500)
    model.RadiationDamping = True
    cpu.set_model(model, 1)
    truth = np.asarray(cpu.forward([1000.0])[1])[:, 0]
    data = truth + 0.01 * np.abs(truth).max() * np.random.default_rng(1).standard_normal(truth.size)
    fn = R.checker_ssq(cpu, data)
    v = [ref.run(lambda q: fn(np.asarray(q).reshape(-1)), [0.0], [1.0e4], 4096, 0.5 * data.size, seed=s)["log_integral"] for s in range(seeds)]
    print(f"specification, real model d = 1: log I {np.mean(v):.4f}, sd {np.std(v, ddof=1):.4f} over {seeds} seeds")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smc", "smc_bench.json"))
    ap.add_argument("--quick", action="store_true", help="the 65 536-particle shapes only, 2 seeds of the whole problem")
    ap.add_argument("--spec-sd", action="store_true")
    a = ap.parse_args()
    if a.spec_sd:
        return spec_sd()
    res = {"build_id": pkg._abi.load().rsf_build_id().decode(), "move": [], "stage": []}
    with pkg.Engine(mem="device") as eng:
        for n in (65536,) if a.quick else (65536, 262144):
            res["move"].append(bench_move(eng, n, 2000))
            res["stage"].append(bench_stage(eng, n))
            print(json.dumps(res["move"][-1]), json.dumps(res["stage"][-1]), flush=True)
    res["whole"] = bench_whole(2 if a.quick else 8)
    print(json.dumps({k: v for k, v in res["whole"].items() if not isinstance(v, list)}))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
