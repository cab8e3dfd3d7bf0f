#!/usr/bin/env python3
"""Cost of rsf_predict_psis_loo against its yardstick, rsf_predict_quantiles with one probability, at the same shape and in the
same process (needs an MI355X; there is no fallback).

    tools/psis_bench.py [--draws 65536 262144] [--nsteps 2000] [--reps 5] [--out profiles/psis/psis_bench.json]

The series is synthetic and stays in device memory (a device-memory Engine): y[k][i] = sin(0.01 k) (1 + 0.1 z_i) + 0.02 e_ki with
standard normal z, e from a seeded generator, data_k = sin(0.01 k) + 0.05 eps_k, std2_i in (0.05^2, 0.3^2) — draws whose
likelihood varies over the rows as a posterior pool's does.  Times are host clocks around calls that end in a stream
synchronise, after one warm-up call of each; the median of --reps.  Run it under rocprofv3 --kernel-trace --stats for the
per-kernel split.  By traffic the new call is 10 reads of the series against 8.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, nargs="+", default=[65536, 262144])
    ap.add_argument("--nsteps", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import bayesian_markov_chain_monte_carlo_amd as pkg

    if not torch.cuda.is_available():
        sys.exit("psis_bench: no GPU visible")
    results = []
    with pkg.Engine(mem="device") as eng:
        dev = f"cuda:{eng.device}"
        for n in a.draws:
            g = torch.Generator(device=dev).manual_seed(n)
            k = torch.arange(a.nsteps, device=dev, dtype=torch.float64)[:, None]
            z = torch.randn(n, device=dev, dtype=torch.float64, generator=g)[None, :]
            series = torch.sin(0.01 * k) * (1.0 + 0.1 * z)
            series += 0.02 * torch.randn(a.nsteps, n, device=dev, dtype=torch.float64, generator=g)
            data = torch.sin(0.01 * k[:, 0]) + 0.05 * torch.randn(a.nsteps, device=dev, dtype=torch.float64, generator=g)
            std2 = (0.05 + 0.25 * torch.rand(n, device=dev, dtype=torch.float64, generator=g)) ** 2
            lpd = np.zeros(a.nsteps)
            torch.cuda.synchronize()

            def timed(fn):
                fn()
                t = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    fn()
                    t.append(time.perf_counter() - t0)
                return float(np.median(t)), t

            # alternate the two so that neither owns a quiet stretch of a shared machine
            tq, tq_all = timed(lambda: eng.predictive_quantiles(series, (0.5,)))
            tp, tp_all = timed(lambda: eng.psis_loo(series, std2, data, lpd))
            tq2, tq2_all = timed(lambda: eng.predictive_quantiles(series, (0.5,)))
            res = eng.psis_loo(series, std2, data, lpd)
            pk = res["pareto_k"]
            r = {"draws": n, "rows": a.nsteps, "series_bytes": 8 * n * a.nsteps, "reps": a.reps,
                 "quantiles_1prob_s": min(tq, tq2), "quantiles_1prob_all_s": tq_all + tq2_all,
                 "psis_loo_s": tp, "psis_loo_all_s": tp_all, "ratio": tp / min(tq, tq2),
                 "psis_effective_GBps": 10 * 8 * n * a.nsteps / tp / 1e9,
                 "n_tail_max": float(res["n_tail"].max()), "pareto_k_quantiles_0_50_90_100": [float(v) for v in np.quantile(pk, [0, 0.5, 0.9, 1])]}
            print(json.dumps(r), flush=True)
            results.append(r)
            del series
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"build_id": eng.lib.rsf_build_id().decode() if hasattr(eng.lib, "rsf_build_id") else None, "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
