#!/usr/bin/env python3
"""Cost of rsf_predict_noise_quantiles against its yardstick, rsf_predict_quantiles with the same probabilities, at the same shape
and in the same process (needs an MI355X; there is no fallback).

    tools/noise_band_bench.py [--draws 65536 262144] [--nsteps 2000] [--reps 5] [--out profiles/noise_band/noise_band_bench.json]

Real draws: Dc uniform in (600, 1600) as in tests/psis_cases.py, std2_i = (u_i amp)^2 with u uniform in (0.05, 0.3) and amp the
largest |y| of the series at Dc = 1000; the series is the one rsf_predict_partials materialises for them and stays in device
memory (a device-memory Engine).  Probabilities (0.05, 0.5, 0.95).  Times are host clocks around calls that end in a stream
synchronise, after one warm-up call of each; the median of --reps.  The yardstick is timed before and after.  The solve that
produced the series (rsf_predict_partials with the series wanted) is timed too.  Run it under rocprofv3 --kernel-trace --stats
for the per-kernel split.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PROBS = (0.05, 0.5, 0.95)


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
        sys.exit("noise_band_bench: no GPU visible")
    results = []
    with pkg.Engine(mem="device") as eng:
        model = pkg.RateStateModel(number_time_steps=a.nsteps)
        model.RadiationDamping = True
        eng.set_model(model, 1)
        truth = np.asarray(eng.forward([1000.0])[1].cpu())[:, 0]
        amp = np.abs(truth).max()
        for n in a.draws:
            rng = np.random.default_rng(n)
            q = rng.uniform(600.0, 1600.0, n)
            data = truth + 0.05 * amp * rng.standard_normal(truth.size)
            std2 = eng._in((rng.uniform(0.05, 0.3, n) * amp) ** 2)
            q = eng._in(q)
            zeros = np.zeros(truth.size)

            def timed(fn):
                fn()
                t = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    fn()
                    t.append(time.perf_counter() - t0)
                return float(np.median(t)), t

            ts, ts_all = timed(lambda: eng.predictive_partials(q, std2, data, truth, zeros, return_series=True))
            series = eng.predictive_partials(q, std2, data, truth, zeros, return_series=True)[1]
            tq, tq_all = timed(lambda: eng.predictive_quantiles(series, PROBS))
            tn, tn_all = timed(lambda: eng.predictive_noise_quantiles(series, std2, PROBS))
            tq2, tq2_all = timed(lambda: eng.predictive_quantiles(series, PROBS))
            band, passes = eng.predictive_noise_quantiles(series, std2, PROBS, return_passes=True)
            clean = eng.predictive_quantiles(series, PROBS)
            rows = series.shape[0]
            evals = float(passes.astype(np.float64).sum() - rows) * n * len(PROBS)  # an upper count: a stopped target costs none
            r = {"draws": n, "rows": rows, "series_bytes": 8 * n * rows, "reps": a.reps, "probs": PROBS,
                 "quantiles_s": min(tq, tq2), "quantiles_all_s": tq_all + tq2_all,
                 "noise_quantiles_s": tn, "noise_quantiles_all_s": tn_all, "ratio": tn / min(tq, tq2),
                 "solve_with_series_s": ts, "solve_with_series_all_s": ts_all, "ratio_to_solve": tn / ts,
                 "passes_mean": float(passes.mean()), "passes_max": int(passes.max()),
                 "traffic_floor_s": float(passes.astype(np.float64).sum()) * 8 * n / 6.3e12,
                 "erfc_exp_evaluations_upper": evals,
                 "noise_band_halfwidth_median": float(np.median(band[2] - band[0]) / 2), "credible_band_halfwidth_median": float(np.median(clean[2] - clean[0]) / 2)}
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
