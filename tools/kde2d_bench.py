#!/usr/bin/env python3
"""Cost of the joint-posterior entry points (include/rsf_joint.h) against their yardsticks, on the same pool and in the same
process (needs an MI355X; there is no fallback).

    tools/kde2d_bench.py [--shapes cfg5 cfg2] [--mesh 64] [--reps 5] [--scipy-samples 20000] [--out profiles/joint/kde2d_bench.json]

Pools (synthetic draws with a joint rate-and-state posterior's scales and correlations, made on the device, kept in device memory):
    cfg5   131 072 chains x 256 kept draws x (Dc, a, b): one GPU's share of BASELINE configs[4]      33.6 M rows, d = 3
    cfg2   262 144 chains x 100 draws x (Dc, sigma^2): configs[2]'s trace with its noise variance    26.2 M rows, d = 2
rsf_pool_kde2d on a mesh x mesh grid over +-4 sd of columns (0, 1) — pairs/s = n m / time — against the 1-D rsf_pool_kde of
column 0 on mesh^2 grid points of the same pool, timed before and after.  rsf_pool_joint_partials and rsf_pool_histogram2d
(40 x 40) as GB/s of the bytes they must read (all d columns; the two columns), against rsf_pool_summary's one column.
Times are host clocks around calls that end in a synchronise, after one warm-up call of each; the median of --reps.
SciPy's gaussian_kde on a subsample of the pool, extrapolated linearly in the sample count as tools/kde_bench.py does.
RSF_HIP_LIB selects another build of the library (the register-tiling variants); the build id is recorded.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"cfg5": (131072 * 256, 3), "cfg2": (262144 * 100, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["cfg5", "cfg2"], choices=sorted(SHAPES))
    ap.add_argument("--mesh", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scipy-samples", type=int, default=20000)
    ap.add_argument("--kde-only", action="store_true", help="the two KDEs only (variant builds)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import bayesian_markov_chain_monte_carlo_amd as pkg

    if not torch.cuda.is_available():
        sys.exit("kde2d_bench: no GPU visible")
    results = []
    with pkg.Engine(mem="device") as eng:

        def timed(fn):
            fn()
            eng.sync()
            t = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                fn()
                eng.sync()
                t.append(time.perf_counter() - t0)
            return float(np.median(t)), t

        for shape in a.shapes:
            n, d = SHAPES[shape]
            g = torch.Generator(device="cuda").manual_seed(n)
            L = torch.tensor([[5.0, 0.0, 0.0], [-0.6e-4, 0.8e-4, 0.0], [0.5e-4, -0.7e-4, 0.5e-4]], dtype=torch.float64, device="cuda")
            x = (torch.randn((n, 3), generator=g, dtype=torch.float64, device="cuda") @ L.T
                 + torch.tensor([1000.0, 0.011, 0.006], dtype=torch.float64, device="cuda"))[:, :d].contiguous()
            mu, sd = x.mean(0).cpu().numpy(), x.std(0).cpu().numpy()
            axes = [np.linspace(mu[i] - 4 * sd[i], mu[i] + 4 * sd[i], a.mesh) for i in (0, 1)]
            pts_h = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 2)
            pts = torch.as_tensor(pts_h, device="cuda")
            m = pts_h.shape[0]
            grid1 = torch.as_tensor(np.linspace(mu[0] - 4 * sd[0], mu[0] + 4 * sd[0], m), device="cuda")
            t1, t1_all = timed(lambda: eng.pool_kde(x, grid1, param=0))
            t2, t2_all = timed(lambda: eng.pool_kde2d(x, pts, params=(0, 1)))
            t1b, t1b_all = timed(lambda: eng.pool_kde(x, grid1, param=0))
            t1 = min(t1, t1b)
            r = {"shape": shape, "rows": n, "d": d, "points": m, "reps": a.reps, "pairs": float(n) * m,
                 "kde1d_s": t1, "kde1d_all_s": t1_all + t1b_all, "kde1d_pairs_per_s": n * m / t1,
                 "kde2d_s": t2, "kde2d_all_s": t2_all, "kde2d_pairs_per_s": n * m / t2, "kde2d_over_kde1d_rate": t1 / t2}
            if not a.kde_only:
                ts, ts_all = timed(lambda: eng.pool_summary(x, 0))
                tj, tj_all = timed(lambda: eng.pool_joint_partials(x))
                ranges = tuple((float(mu[i] - 4 * sd[i]), float(mu[i] + 4 * sd[i])) for i in (0, 1))
                th, th_all = timed(lambda: eng.pool_histogram2d(x, 40, ranges))
                tb, tb_all = timed(lambda: eng.pool_histogram2d(x, 126, ranges))
                t1h, _ = timed(lambda: eng.pool_histogram(x, 40, ranges[0][0], ranges[0][1], param=0))
                r.update({"summary_s": ts, "summary_GBps": 8e-9 * n / ts, "summary_all_s": ts_all,
                          "joint_partials_s": tj, "joint_partials_GBps": 8e-9 * n * d / tj, "joint_partials_all_s": tj_all,
                          "histogram2d_40_s": th, "histogram2d_40_GBps": 16e-9 * n / th, "histogram2d_40_all_s": th_all,
                          "histogram2d_126_s": tb, "histogram2d_126_GBps": 16e-9 * n / tb, "histogram2d_126_all_s": tb_all,
                          "histogram1d_40_s": t1h, "histogram1d_40_GBps": 8e-9 * n / t1h, "block_bytes": 8 * n * d})
                if a.scipy_samples > 0:
                    from scipy.stats import gaussian_kde

                    sub = x[:: max(1, n // a.scipy_samples), :2].cpu().numpy()
                    t0 = time.perf_counter()
                    ref = gaussian_kde(sub.T)(pts_h.T)
                    tsp = time.perf_counter() - t0
                    dens = eng.pool_kde2d(x, pts, params=(0, 1)).cpu().numpy()
                    r.update({"scipy_samples": int(sub.shape[0]), "scipy_s": tsp, "scipy_pairs_per_s": sub.shape[0] * m / tsp,
                              "scipy_extrapolated_to_pool_s": tsp * n / sub.shape[0],
                              "max_abs_density_diff_vs_subsample_kde_over_max": float(np.abs(dens - ref).max() / dens.max())})
            print(json.dumps(r), flush=True)
            results.append(r)
            del x
            torch.cuda.empty_cache()
        build = eng.lib.rsf_build_id().decode()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"build_id": build, "lib": os.environ.get("RSF_HIP_LIB") and os.path.basename(os.path.dirname(os.environ["RSF_HIP_LIB"])),
                       "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
