#!/usr/bin/env python3
"""
rank_diag_bench.py — time the rank-normalised diagnostics (Engine.rank_diagnostics: rsf_diag_rank_prepare, the lag-block loop of
rsf_diag_rank_partials + rsf_diag_rank_finish) at the shapes the sampler produces, next to the sort's HBM floor and to the NumPy
restatement (tests/rank_diagnostics_reference.py in float64).

  python tools/rank_diag_bench.py [--shapes 100x262144x1,4000x131072x3] [--numpy-max-gb 1] [--reps 3]

The traces are synthetic and made on the device, as in tools/diag_bench.py: AR(1) chains with phi = 0.9, 1 % of the chains frozen
at their start.  Per shape, one JSON line:
  wall_ms          one Engine.rank_diagnostics call on a device-resident trace (sorts, series, lag blocks), best of --reps;
  prepare_ms       rsf_diag_rank_prepare alone (two sorts per parameter, the ranks, order statistics and indicators), best of --reps;
  lags             lags the default call computed (all four series to Geyer's truncation);
  sort_floor_ms    one parameter's sort at 8 passes: (key pass 20 B + 8 passes x 32 B) per draw / 6.3 TB/s;
  workspace_gb     the rank workspace: the four series (4 x trace) + 24 B per draw of sort buffers (+ tile arrays);
  numpy_s          the float64 NumPy/SciPy restatement at the same shape (skipped above --numpy-max-gb of trace).
Kernel times (the sort's passes among them) come from a run of its own under `rocprofv3 --kernel-trace --stats`.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_TBS = 6.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="100x262144x1,4000x131072x3")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--numpy-max-gb", type=float, default=1.0)
    a = ap.parse_args()
    import torch

    import bayesian_markov_chain_monte_carlo_amd as pkg
    from diag_bench import make_trace

    with pkg.Engine(mem="device") as eng:  # warm-up: load every kernel once
        eng.rank_diagnostics(make_trace(torch, 16, 1024, 3, seed=1))
    for shape in a.shapes.split(","):
        n, C, d = (int(v) for v in shape.split("x"))
        x = make_trace(torch, n, C, d)
        torch.cuda.synchronize()
        A = n * C
        ntiles = -(-A // 4096)
        rec = dict(shape=[n, C, d], trace_gb=x.numel() * 8 / 1e9,
                   workspace_gb=(4 * A * d * 8 + A * 24 + ntiles * 259 * 4) / 1e9,
                   sort_floor_ms=A * (20 + 8 * 32) / (HBM_TBS * 1e12) * 1e3)
        with pkg.Engine(mem="device") as eng:
            best, prep = None, None
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eng.rank_prepare(x)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                eng.rank_release()
                prep = dt if prep is None else min(prep, dt)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = eng.rank_diagnostics(x)
                dt = time.perf_counter() - t0
                best = dt if best is None else min(best, dt)
            rec.update(wall_ms=best * 1e3, prepare_ms=prep * 1e3, lags=res[0]["n_lags"],
                       rhat=[r["rhat"] for r in res], ess_bulk=[r["ess_bulk"] for r in res], ess_tail=[r["ess_tail"] for r in res],
                       median=[r["median"] for r in res], lags_complete=[r["lags_complete"] for r in res])
        if rec["trace_gb"] <= a.numpy_max_gb:
            import diagnostics_reference as dref
            import rank_diagnostics_reference as rref

            dref.LD = np.float64  # the restatement in plain float64: what a NumPy user would run
            h = x.cpu().numpy()
            t0 = time.perf_counter()
            rref.rank_diagnostics(h)
            rec["numpy_s"] = time.perf_counter() - t0
            del h
        del x
        torch.cuda.empty_cache()
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
