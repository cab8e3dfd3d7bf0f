#!/usr/bin/env python3
"""Cost and behaviour of the marginal-likelihood entry points (include/rsf_evidence.h) on one MI355X.

  time   Engine.evidence end to end at --draws x --nsteps (d = 1, device memory), and evidence_logtarget alone against the bare
         forward solve with SSq (rsf_forward_batch) of the same points: best of --repeat wall-clock times around a synchronise.
  fits   the Dc-only fit against the (Dc, a, b) fit of one data set (nsteps 500, 4096 chains, n0 = 0): re and n2_in_box of the
         d = 3 evidence with the identity transform and with log on (Dc, a), and the log Bayes factor of d = 1 against d = 3.

Prints one JSON object; --out writes it to a file as well."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bayesian_markov_chain_monte_carlo_amd as pkg  # noqa: E402


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


def time_leg(draws, nsteps, repeat):
    model = pkg.RateStateModel(number_time_steps=nsteps)
    model.RadiationDamping = True
    out = {}
    with pkg.Engine(mem="device") as eng:
        eng.set_model(model, 1)
        _, acc = eng.forward([1000.0])
        acc = acc[:, 0].cpu().numpy()
        rng = np.random.default_rng(1)
        data = acc + np.abs(acc) * rng.standard_normal(acc.size)
        for n in draws:
            q = eng._in(rng.normal(1000.0, 30.0, (n, 1)))
            logg = eng._in(np.zeros(n))
            obs = eng._in(data)
            col = q[:, 0].contiguous()
            t_l = best(lambda: eng.evidence_logtarget(q, obs, 0.0, 1e4, logg), eng.sync, repeat)
            t_f = best(lambda: eng.forward(col, data=obs, want_ssq=True, want_acc=False), eng.sync, repeat)
            t_e = best(lambda: eng.evidence(q, obs, 0.0, 1e4), eng.sync, max(2, repeat // 2))
            res = eng.evidence(q, obs, 0.0, 1e4)
            out[str(n)] = {"evidence_ms": t_e, "logtarget_ms": t_l, "forward_ssq_ms": t_f, "logtarget_over_forward": t_l / t_f,
                           "iterations": res["iterations"], "re": res["re"], "n2_in_box": res["n2_in_box"]}
    return out


def fits_leg(chains, nsamples, seed):
    model = pkg.RateStateModel(number_time_steps=500)
    model.RadiationDamping = True
    with pkg.Engine(mem="host") as eng:
        eng.set_model(model, 1)
        _, acc = eng.forward([1000.0])
        truth = np.asarray(acc)[:, 0]
    data = truth + 0.01 * np.abs(truth).max() * np.random.default_rng(1).standard_normal(truth.size)
    lo3, hi3 = [0.0, 0.005, 0.005], [1.0e4, 0.02, 0.03]
    out = {}
    mc1 = pkg.MCMC(model, data, 1000.0, ["Uniform", 0.0, 1.0e4], 1000.0, nsamples=nsamples, verbose=False)
    mc1.n0 = 0.0
    p1 = mc1.sample_batched(chains, seed=seed)
    e1 = p1.evidence(model, data, [0.0], [1.0e4])
    out["d1"] = {k: e1[k] for k in ("log_evidence", "log_integral", "re", "n2_in_box", "n2", "ess_factor", "iterations", "converged")}
    mc3 = pkg.MCMC(model, data, 1000.0, [["Uniform", l, h] for l, h in zip(lo3, hi3)], [1000.0, model.a, model.b], nsamples=nsamples,
                   verbose=False)
    mc3.n0 = 0.0
    p3 = mc3.sample_batched(chains, seed=seed)
    lo3[0] = 1e-3  # the log transform needs lo > 0; no draw lies below (Dc < 0.35 has no finite series)
    for name, tr in (("identity", ("identity",) * 3), ("log_Dc_a", ("log", "log", "identity"))):
        e3 = p3.evidence(model, data, lo3, hi3, transform=tr)
        out["d3_" + name] = {k: e3[k] for k in ("log_evidence", "log_integral", "re", "n2_in_box", "n2", "ess_factor", "iterations", "converged")}
        out["log_bf_d1_over_d3_" + name] = pkg.bayes_factor(e1, e3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--draws", type=int, nargs="*", default=[65536, 262144])
    ap.add_argument("--nsteps", type=int, default=2000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--fits", action="store_true")
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--nsamples", type=int, default=400)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()
    res = {"build_id": pkg._abi.load().rsf_build_id().decode(), "nsteps": a.nsteps}
    if a.draws:
        res["time"] = time_leg(a.draws, a.nsteps, a.repeat)
    if a.fits:
        res["fits"] = fits_leg(a.chains, a.nsamples, a.seed)
    text = json.dumps(res, indent=1, default=float)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
