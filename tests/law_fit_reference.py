"""
The specification of the Levenberg-Marquardt fit under a state law (include/rsf_law_fit.h), a test helper (TEST INFRASTRUCTURE ONLY):
tests/fit_reference.py's `normal` and `fit` with a `solve` made from tests/observe_reference.forward, in float64 or long double.
No algorithm of its own: the normal equations, the iteration, the statuses and the constants are fit_reference's, the series
observe_reference's.

What tests/test_law_fit_reference.py (CPU) and tests/test_gpu_law_fit.py share is here too: the problems of the end-to-end tests and
the specification's fits of them, solved ONCE per process.
"""
import functools

import numpy as np

import fit_reference as F
import law_cases as C
import law_dr_reference as S
import law_reference as R
import observe_cases as OC
import observe_reference as O

FD = {1: 1e-6, 3: 1e-4}  # Engine.fit's default forward-difference steps
BOX = {1: (np.array([R.BF_BOX[0]]), np.array([R.BF_BOX[1]])), 3: (S.LO3, S.HI3)}
# the end-to-end starts: d = 1 across the box on both sides of the truth (Dc = 20); d = 3 a handful inside the box around it
STARTS1 = (8.0, 14.0, 30.0, 60.0, 150.0)
STARTS3 = ((15.0, 0.0105, 0.0135), (25.0, 0.0115, 0.0145), (18.0, 0.0112, 0.0138), (30.0, 0.0100, 0.0150))


def solve(m, vl, law, observable, dtype=np.float64):
    """fit_reference's solve: points (n, 1) of Dc or (n, 3) of (Dc, a, b) -> the series (nout, n) of `observable` in `dtype`"""

    def run(points):
        p = np.asarray(points, dtype=np.float64)
        a, b = (p[:, 1], p[:, 2]) if p.shape[1] == 3 else (None, None)
        return O.forward(m, p[:, 0], vl, law, observable, a=a, b=b, dtype=dtype)[0]

    return run


def normal(m, vl, law, observable, q, data, fd, dtype=np.float64, out=np.float64):
    """fit_reference.normal on the state-law series -> (ssq (n,), grad (n, d), jtj (n, d, d)) of dtype `out`"""
    return F.normal(solve(m, vl, law, observable, dtype), np.asarray(q, dtype=np.float64).reshape(len(q), -1), data, fd, out)


def fit(m, vl, law, observable, q0, data, lo, hi, fd, dtype=np.float64, ftol=F.FTOL, max_iter=100, history=None):
    """fit_reference.fit on the state-law series -> its state dict"""
    s = solve(m, vl, law, observable, dtype)
    return F.fit(lambda p: F.normal(s, p, data, fd), q0, lo, hi, ftol, max_iter, history)


@functools.lru_cache(maxsize=None)
def fit_d1(truth):
    """observe_cases.friction_problem(truth) fitted in Dc from STARTS1 under the true law by the float64 specification"""
    p = OC.friction_problem(truth)
    return fit(p["m"], p["vl"], truth, "mu", np.array(STARTS1)[:, None], p["data"], *BOX[1], FD[1], max_iter=60)


@functools.lru_cache(maxsize=None)
def fit_d3(truth):
    """the same data fitted in (Dc, a, b) from STARTS3"""
    p = OC.friction_problem(truth)
    return fit(p["m"], p["vl"], truth, "mu", np.array(STARTS3), p["data"], *BOX[3], FD[3], max_iter=60)
