#!/usr/bin/env python3
"""Cost of the posterior predictive checks on the MI355X, in one process:

  (a) rsf_forward_batch with ssq_out only on n draws at nsteps 2000: the yardstick, its kernel is the sampler's solve;
  (b) rsf_predict_partials without the series on the same draws;
  (c) with --band N: the series-plus-quantiles path on N draws (rsf_predict_partials with the series, rsf_predict_quantiles),
      the select kernel's traffic floor (8 reads of the series at 6.3 TB/s) and the same statistics in NumPy on the host.

Wall times are host-side, device-memory engine, synchronised; kernel times come from a separate run of this script under
rocprofv3 --kernel-trace --stats.  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bayesian_markov_chain_monte_carlo_amd as pkg  # noqa: E402


def timed(fn, sync, reps):
    fn()
    sync()
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        best = min(best, time.perf_counter() - t0)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=262144)
    ap.add_argument("--nsteps", type=int, default=2000)
    ap.add_argument("--substeps", type=int, default=1)
    ap.add_argument("--band", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--numpy", action="store_true", help="also time the same statistics in NumPy on the host (band draws)")
    args = ap.parse_args()
    import torch

    model = pkg.RateStateModel(number_time_steps=args.nsteps)
    rng = np.random.default_rng(3)
    out = {"draws": args.draws, "nsteps": args.nsteps, "substeps": args.substeps, "band_draws": args.band}
    with pkg.Engine(mem="device") as e:
        e.set_model(model, args.substeps)
        sync = torch.cuda.synchronize
        _, acc = e.forward([1000.0])
        truth = acc[:, 0].cpu().numpy()
        sigma0 = 0.01 * np.abs(truth).max()
        data = truth + sigma0 * rng.standard_normal(truth.size)
        q = e._in(rng.normal(1000.0, 5.0, args.draws))
        s2 = e._in(rng.uniform(0.8, 1.25, args.draws) * sigma0 ** 2)
        cy = truth
        cl = -0.5 * np.log(2 * np.pi * sigma0 ** 2) - (data - cy) ** 2 / (2 * sigma0 ** 2)
        d_data = e._in(data)
        out["forward_ssq_s"] = timed(lambda: e.forward(q, data=d_data, want_ssq=True, want_acc=False), sync, args.reps)
        out["predict_partials_s"] = timed(lambda: e.predictive_partials(q, s2, d_data, cy, cl), sync, args.reps)
        out["ratio"] = out["predict_partials_s"] / out["forward_ssq_s"]
        if args.band > 0:
            qb, sb = q[:args.band], s2[:args.band]
            probs = (0.05, 0.5, 0.95)
            out["band_partials_series_s"] = timed(lambda: e.predictive_partials(qb, sb, d_data, cy, cl, return_series=True), sync, args.reps)
            part, series = e.predictive_partials(qb, sb, d_data, cy, cl, return_series=True)
            out["band_quantiles_s"] = timed(lambda: e.predictive_quantiles(series, probs), sync, args.reps)
            out["select_traffic_floor_s"] = 8 * series.numel() * 8 / 6.3e12
            if args.numpy:
                h, hs = series.cpu().numpy(), sb.cpu().numpy()
                t0 = time.perf_counter()
                r = data[:, None] - h
                l = -0.5 * np.log(2 * np.pi * hs)[None, :] - r * r / (2 * hs)[None, :]
                from scipy.special import ndtr
                stats = (h.mean(1), h.var(1, ddof=1), ndtr(r / np.sqrt(hs)[None, :]).mean(1), np.log(np.exp(l - cl[:, None]).mean(1)) + cl,
                         l.var(1, ddof=1), np.quantile(h, probs, axis=1))
                out["numpy_host_s"] = time.perf_counter() - t0
                del stats
    print(json.dumps(out))


if __name__ == "__main__":
    main()
