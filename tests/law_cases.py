"""
What tests/test_law_reference.py (CPU) and tests/test_gpu_law.py share (a test helper): the precision lane sets with the float64
and the long-double specification solved ONCE per process (tests/law_reference.py), and the Bayes-factor data sets.
"""
import functools

import numpy as np

import law_reference as R

WAVE = 64
CAP = 1e-9  # the project's Tier-1 bound on a float64 RK4 trajectory: rtol 1e-9 of the lane's max|acc|
LOW = (2.0, 3.0)  # the step history's stable lanes below the precision set, ageing law (the slip law's RK4 is not finite there)


def spec(nsteps=500, substeps=1, **attrs):
    m = R.Spec(nsteps, 0.0, 50.0, substeps)
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


def padded(lanes):
    """the lanes, then Dc = 1000 up to whole waves of 64"""
    lanes = np.asarray(lanes, dtype=np.float64)
    return np.concatenate([lanes, np.full(-lanes.size % WAVE, 1000.0)])


@functools.lru_cache(maxsize=None)
def precision_set(history, law, low=False):
    """One lane set of the precision tests at nsteps 500, substeps 1: R.LANES (low: LOW first) under `history` and `law` →
    dict(dc, vl, acc (float64 specification), ext (long double), err (per lane: the float64 specification's distance from the
    long-double one relative to the lane's max|acc|), yardstick = err.max())"""
    m = spec()
    dc = np.asarray((LOW if low else ()) + R.LANES)
    vl = R.table(m, history)
    acc, _ = R.forward(m, dc, vl, law)
    ext, _ = R.forward(m, dc, vl, law, dtype=R.LD)
    assert np.isfinite(ext.astype(np.float64)).all(), (history, law)
    err = R.rel_error(acc, ext)
    return {"m": m, "dc": dc, "vl": vl, "acc": acc, "ext": ext, "err": err, "yardstick": float(err.max())}


@functools.lru_cache(maxsize=None)
def bayes_factor_problem(truth):
    """The step-history data set whose truth is `truth` (Dc = 20, noise 5 % of max|clean|) with the float64 specification's
    log evidences on 4001 uniform trapezoid nodes over [5, 200] → dict(m, vl, data, log_evidence {law: .}, ssq {law: .},
    log_bayes_factor = slip - ageing)"""
    m = spec()
    vl = R.table(m, "step")
    data = R.bf_data(m, vl, truth)
    ev, ssq = R.bf_log_evidences(m, vl, data)
    return {"m": m, "vl": vl, "data": data, "log_evidence": ev, "ssq": ssq, "log_bayes_factor": ev["slip"] - ev["aging"]}
