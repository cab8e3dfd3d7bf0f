#!/usr/bin/env python3
"""The reference quadrature's own resolution distance at d = 3 (no GPU): posterior_reference.grid_shift_in_se between Posterior3
at its defaults and at (n_ab 48, n_pc 193), at C = 262 144, on the CPU checker in the box and with the observation of
tests/test_gpu_posterior.py → tests/golden/grid_self_distance.json.  tests/test_gpu_grid.py holds the GPU quadrature to 8 x this
table (0.25 SE where it is smaller); DESIGN.md 4l quotes it.  About 550 000 checker solves."""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ["RSF_ALLOW_CHECKER_ENGINE"] = "1"
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import bayesian_markov_chain_monte_carlo_amd as pkg  # noqa: E402
import posterior_reference as R  # noqa: E402
import rsf_oracle  # noqa: E402
from conftest import synthetic_data  # noqa: E402

LO3, HI3, C = [0.0, 0.005, 0.005], [1.0e4, 0.02, 0.03], 262144


def main():
    eng = pkg.Engine(lib=pkg._abi.bind(ctypes.CDLL(rsf_oracle.build())), checker=True)
    model = pkg.RateStateModel(number_time_steps=500)
    model.RadiationDamping, model.precision, model.integrator = True, "float64", "rk4"
    eng.set_model(model, 1)
    data = synthetic_data(eng)
    fn = R.checker_ssq(eng, data)
    r1 = R.Posterior3(fn, LO3, HI3, 0.5 * data.size)
    r2 = R.Posterior3(fn, LO3, HI3, 0.5 * data.size, n_ab=48, n_pc=193)
    shift = R.grid_shift_in_se(r1, r2, C)
    out = {"C": C, "box": [LO3, HI3], "nsteps": 500, "defaults": {"n_ab": 32, "n_pc": 97}, "finer": {"n_ab": 48, "n_pc": 193},
           "shift_in_se": {k: float(v) for k, v in shift.items()}}
    print(json.dumps(out, indent=1))
    with open(os.path.join(ROOT, "tests", "golden", "grid_self_distance.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
