#!/usr/bin/env python3
"""Cost of the grid posterior (include/rsf_grid.h) on one MI355X, device memory, one process.

  kernel     rsf_grid_logtarget against rsf_evidence_logtarget on the same points in the same order — a (1024, 128, 2) and a
             (2001, 65, 65) grid, 262 144 and 8.5 M nodes — at nsteps 500 and 2000: best of --repeat wall-clock times around a
             synchronise; the evidence kernel is timed before and after the grid kernel.
  undamped   the same comparison at D = 3 without radiation damping, plain and product coordinates (the instantiations whose register
             count differs from the damped ones: profiles/grid/resource_report.txt), on the 8.5 M-node grid, nsteps 500.
  posterior  Engine.grid_posterior end to end at both defaults (d = 1: (4001,), d = 3: (2001, 65, 65)), nsteps 500, and its parts:
             the fine grid's solve, the reductions, finish, 262 144 draws with their sigma^2.
  draws      effective draws per forward solve: n independent draws cost the grid's solves once and one solve each.

Prints one JSON object; --out writes it to a file as well."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bayesian_markov_chain_monte_carlo_amd as pkg  # noqa: E402

LO3, HI3 = [0.0, 0.005, 0.005], [1.0e4, 0.02, 0.03]


def best(fn, sync, repeat):
    fn()
    sync()
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append(time.perf_counter() - t0)
    return min(ts) * 1e3


def observation(eng):
    _, acc = eng.forward([1000.0])
    acc = acc[:, 0].cpu().numpy()
    return acc + np.abs(acc) * np.random.default_rng(2025).standard_normal(acc.size)


def kernel_leg(nsteps_list, repeat):
    out = {}
    grids = {"262144": [np.linspace(300.0, 3000.0, 1024), np.linspace(0.006, 0.019, 128), np.array([0.02, 0.021])],
             "8454225": [np.linspace(300.0, 3000.0, 2001), np.linspace(0.006, 0.019, 65), np.linspace(0.008, 0.028, 65)]}
    for nsteps in nsteps_list:
        model = pkg.RateStateModel(number_time_steps=nsteps)
        model.RadiationDamping = True
        with pkg.Engine(mem="device") as eng:
            eng.set_model(model, 1)
            obs = eng._in(observation(eng))
            for name, x in grids.items():
                q = eng._in(np.stack([np.ravel(a, order="F") for a in np.meshgrid(*x, indexing="ij")], axis=1))
                n = int(q.shape[0])
                logg = eng._in(np.zeros(n))
                t_e0 = best(lambda: eng.evidence_logtarget(q, obs, LO3, HI3, logg), eng.sync, repeat)
                t_g = best(lambda: eng.grid_logtarget(x, obs, LO3, HI3), eng.sync, repeat)
                t_e1 = best(lambda: eng.evidence_logtarget(q, obs, LO3, HI3, logg), eng.sync, repeat)
                out[f"nsteps{nsteps}_n{n}"] = {"grid_logtarget_ms": t_g, "evidence_logtarget_ms_before": t_e0, "evidence_logtarget_ms_after": t_e1,
                                               "grid_over_evidence": t_g / min(t_e0, t_e1), "rk4_steps_per_s": n * nsteps / (t_g * 1e-3)}
    return out


def undamped_leg(repeat, nsteps=500):
    """grid_logtarget_kernel<3, false, plain / product> against evidence_logtarget_kernel<3, false> on the same points"""
    out = {}
    model = pkg.RateStateModel(number_time_steps=nsteps)
    model.RadiationDamping = False
    grids = {"plain": [np.linspace(300.0, 3000.0, 2001), np.linspace(0.006, 0.019, 65), np.linspace(0.008, 0.028, 65)],
             "product": [np.linspace(4.0, 40.0, 2001), np.linspace(0.006, 0.019, 65), np.linspace(0.008, 0.028, 65)]}
    with pkg.Engine(mem="device") as eng:
        eng.set_model(model, 1)
        obs = eng._in(observation(eng))
        for coords, x in grids.items():
            pts = np.stack([np.ravel(a, order="F") for a in np.meshgrid(*x, indexing="ij")], axis=1)
            if coords == "product":
                pts[:, 0] /= pts[:, 1]
            q = eng._in(pts)
            logg = eng._in(np.zeros(pts.shape[0]))
            t_e0 = best(lambda: eng.evidence_logtarget(q, obs, LO3, HI3, logg), eng.sync, repeat)
            t_g = best(lambda: eng.grid_logtarget(x, obs, LO3, HI3, coords), eng.sync, repeat)
            t_e1 = best(lambda: eng.evidence_logtarget(q, obs, LO3, HI3, logg), eng.sync, repeat)
            out[coords] = {"nodes": int(pts.shape[0]), "nsteps": nsteps, "grid_logtarget_ms": t_g, "evidence_logtarget_ms_before": t_e0,
                           "evidence_logtarget_ms_after": t_e1, "grid_over_evidence": t_g / min(t_e0, t_e1)}
    return out


def posterior_leg(repeat, n_draws):
    out = {}
    model = pkg.RateStateModel(number_time_steps=500)
    model.RadiationDamping = True
    with pkg.Engine(mem="device") as eng:
        eng.set_model(model, 1)
        data = observation(eng)
        obs = eng._in(data)
        for d, lo, hi in ((1, [0.0], [1.0e4]), (3, LO3, HI3)):
            post = eng.grid_posterior(obs, lo, hi)
            t_all = best(lambda: eng.grid_posterior(obs, lo, hi), eng.sync, repeat)
            coords = post.coords
            t_solve = best(lambda: eng.grid_logtarget(post.x, obs, lo, hi, coords), eng.sync, repeat)
            l, ssq = eng.grid_logtarget(post.x, obs, lo, hi, coords)
            t_col = best(lambda: eng.grid_columns(post.x, post.w, l, ssq), eng.sync, repeat)
            t_fin = best(lambda: eng.grid_finish(post.x, post.w, lo, hi, post.shape, post.lmax, post.fields, post.x[0][post.n[0] // 2], coords), eng.sync, repeat)
            t_draw = best(lambda: post.draw(n_draws, seed=1), eng.sync, repeat)
            t_cdf = best(lambda: eng.grid_cdf(post.x, post.cum0, post.finish["pair"], np.linspace(lo[0], hi[0], 4001), coords), eng.sync, repeat)
            t_dc = best(lambda: post.dc_cdf(np.linspace(lo[0], hi[0], 4001)), eng.sync, repeat) if d == 3 else None
            out[f"d{d}"] = {"n": list(post.n), "dc_cdf_refined_4001_ms": t_dc, "n_solves": post.n_solves, "grid_posterior_ms": t_all, "fine_solve_ms": t_solve, "columns_ms": t_col,
                            "finish_ms": t_fin, f"draw_{n_draws}_ms": t_draw, "cdf_4001_ms": t_cdf, "outside": post.outside,
                            "log_evidence": post.log_evidence, "mean": list(post.mean), "sd": list(np.sqrt(np.diag(post.cov))),
                            "std2_mean": post.std2_mean, "n_neginf": post.n_neginf,
                            # n independent draws: the grid's solves once, one solve per draw for sigma^2
                            "effective_draws_per_solve": {str(n): n / (post.n_solves + n) for n in (65536, 262144, 1048576)}}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nsteps", type=int, nargs="*", default=[500, 2000])
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--draws", type=int, default=262144)
    ap.add_argument("--out")
    a = ap.parse_args()
    res = {"build_id": pkg._abi.load().rsf_build_id().decode(), "kernel": kernel_leg(a.nsteps, a.repeat), "undamped": undamped_leg(a.repeat), "posterior": posterior_leg(a.repeat, a.draws)}
    text = json.dumps(res, indent=1, default=float)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
