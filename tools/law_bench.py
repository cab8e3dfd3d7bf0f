#!/usr/bin/env python3
"""
Cost of the plain float64 solve under either state law (include/rsf_law.h, rsf_law_forward) against the tier kernels
(rsf_forward_batch) on the GPU: recorded, not gated.
    python tools/law_bench.py [--out profiles/law/law_bench.json] [--quick]
One process, device-memory engine, SSq mode (no series), the same 65 536 points (Dc log-uniform over [300, 5000]: the TIGHT tier of
the incremental step) at nsteps 2000 under the built-in history.  Each of the three calls is warmed up, then the three are timed in
turn, `rounds` times over, each timing a host clock around `reps` calls (64: a window of 25 ms for the fastest of the three, so
that neither the clock nor one call's host overhead carries weight) that ends in a device synchronise; reported: the median
over the rounds, the spread (min, max) and the ratios of the medians.  Before any timing the three results are compared on the same
points.  Beside the ratio: the VALU instructions per RK4 step as compiled, counted in the library's own code object — for
law_forward_kernel four times its stage loop plus the step's remainder; for the incremental tiers DESIGN.md 4's table.
"""
import argparse
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import bayesian_markov_chain_monte_carlo_amd as pkg  # noqa: E402
import kernel_diff  # noqa: E402

TIER_VALU = {"TIGHT": 87.6, "NARROW": 104.5, "WIDE": 122.0}  # VALU per step of the damped incremental tiers outside the sampler


def valu_per_step(lib_path):
    """{kernel: (VALU in the stage loop, VALU in the step loop outside it, VALU per step)} of the law_forward_kernel instances.
    A listing line's size is four bytes per word of its encoding comment, which places every line and every branch target; the
    stage loop is the loop without an inner loop that holds the most VALU instructions, the step loop the smallest loop around it."""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        listing = kernel_diff.kernels(lib_path, tmp, "lib")
    for name, lines in listing.items():
        if "law_forward_kernel" not in name:
            continue
        addr, at = [], 0
        for line in lines:
            addr.append(at)
            enc = line.split("//")[1].split("<")[0] if "//" in line else ""
            at += 4 * len(re.findall(r"\b[0-9A-F]{8}\b", enc))
        loops = []
        for i, line in enumerate(lines):
            m = re.search(r"^\s*s_c?branch\S*\s.*<.*\+0x([0-9a-f]+)>", line)
            if m and int(m.group(1), 16) <= addr[i]:
                loops.append((addr.index(int(m.group(1), 16)), i))
        valu = lambda a, b: sum(1 for line in lines[a:b + 1] if line.strip().startswith("v_"))
        inner = [lp for lp in loops if not any(o != lp and lp[0] <= o[0] and o[1] <= lp[1] for o in loops)]
        stage = max(inner, key=lambda lp: valu(*lp))
        step = min((lp for lp in loops if lp != stage and lp[0] <= stage[0] and stage[1] <= lp[1]), key=lambda lp: lp[1] - lp[0])
        rest = valu(*step) - valu(*stage)
        out[name] = (valu(*stage), rest, 4 * valu(*stage) + rest)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="4096 points, nsteps 500")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=64, help="calls per timed window: 64 make the shortest window about 25 ms")
    args = ap.parse_args()
    n, nsteps = (4096, 500) if args.quick else (65536, 2000)
    lib = pkg._abi.load()
    out = {"device": None, "build_id": lib.rsf_build_id().decode(), "n": n, "nsteps": nsteps, "rounds": args.rounds, "reps": args.reps}
    counts = valu_per_step(pkg._abi.LIB_PATH)
    out["valu_per_step"] = {("slip" if "ILi1E" in k else "aging") + (", damped" if "Lb1E" in k else ", undamped"): dict(zip(("stage_loop", "step_remainder", "per_step"), v))
                            for k, v in counts.items()}
    out["valu_per_step"]["incremental tiers (DESIGN.md 4, damped)"] = TIER_VALU
    import torch

    with pkg.Engine(mem="device") as eng:
        out["device"] = torch.cuda.get_device_name(eng.device)
        eng.set_model(pkg.RateStateModel(number_time_steps=nsteps), 1)
        truth = np.asarray(eng.forward([1000.0])[1].cpu())[:, 0]
        data = eng._in(truth + 0.01 * np.abs(truth).max() * np.random.default_rng(1).standard_normal(truth.size))
        dc = eng._in(np.exp(np.random.default_rng(2).uniform(np.log(300.0), np.log(5000.0), n)))
        calls = {"forward_batch": lambda: eng.forward(dc, data=data, want_ssq=True, want_acc=False)[0],
                 "law_forward_aging": lambda: eng.law_forward("aging", dc, data=data, want_ssq=True, want_acc=False)[0],
                 "law_forward_slip": lambda: eng.law_forward("slip", dc, data=data, want_ssq=True, want_acc=False)[0]}
        res = {k: np.asarray(f().cpu()) for k, f in calls.items()}  # the warm-up of every shape timed, and the results
        eng.sync()
        out["ssq_aging_vs_forward_batch"] = float((np.abs(res["law_forward_aging"] - res["forward_batch"]) / res["forward_batch"]).max())
        out["ssq_slip_vs_aging"] = float((np.abs(res["law_forward_slip"] - res["law_forward_aging"]) / res["law_forward_aging"]).max())
        times = {k: [] for k in calls}
        for _ in range(args.rounds):
            for k, f in calls.items():  # in turn, so that a drift of the machine touches all three alike
                eng.sync()
                t = time.perf_counter()
                for _ in range(args.reps):
                    f()
                eng.sync()
                times[k].append((time.perf_counter() - t) / args.reps)
    steps = n * (nsteps - 1)
    for k, ts in times.items():
        out[k] = {"median_s": float(np.median(ts)), "min_s": float(min(ts)), "max_s": float(max(ts)), "ns_per_lane_step": float(np.median(ts)) / steps * 1e9}
    base = out["forward_batch"]["median_s"]
    damped = out["valu_per_step"]
    for law in ("aging", "slip"):
        out[f"law_forward_{law}"]["over_forward_batch"] = out[f"law_forward_{law}"]["median_s"] / base
        out[f"law_forward_{law}"]["valu_over_tight"] = damped[f"{law}, damped"]["per_step"] / TIER_VALU["TIGHT"]
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
